// fpfh_table.h -- K16: the sector boundaries of the first FPFH feature (include/icpk.h, "B1").  Row k - 1 holds
// {C_k, S_k}, the doubles nearest cos(beta_k) and sin(beta_k) for beta_k = -pi + 2 pi k / 11, k = 1 .. 10 (computed
// with 200-bit arithmetic, then rounded once).  The device (kernels_fpfh.hip) includes this file; the CPU model
// (tests/fpfh_model.py) parses the same hex literals out of it, so both sides compare against the same bits.
#pragma once

namespace icpk {

constexpr double FPFH_CS[10][2] = {
    /* k =  1 */ {-0x1.aeb8c8764f0bap-1, -0x1.14cedf8bb580bp-1},  /* -0.84125353283118121 -0.54064081745559756 */
    /* k =  2 */ {-0x1.a9628d9c712b6p-2, -0x1.d1bb48eee2c13p-1},  /* -0.41541501300188644 -0.90963199535451833 */
    /* k =  3 */ {0x1.2375f640f44dbp-3, -0x1.fac9e043842efp-1},   /* +0.14231483827328514 -0.98982144188093268 */
    /* k =  4 */ {0x1.4f49e7f775887p-1, -0x1.82f19bb3a28a1p-1},   /* +0.65486073394528510 -0.75574957435425827 */
    /* k =  5 */ {0x1.eb42a9bcd5057p-1, -0x1.207e7fd768dbfp-2},   /* +0.95949297361449737 -0.28173255684142967 */
    /* k =  6 */ {0x1.eb42a9bcd5057p-1, 0x1.207e7fd768dbfp-2},    /* +0.95949297361449737 +0.28173255684142967 */
    /* k =  7 */ {0x1.4f49e7f775887p-1, 0x1.82f19bb3a28a1p-1},    /* +0.65486073394528510 +0.75574957435425827 */
    /* k =  8 */ {0x1.2375f640f44dbp-3, 0x1.fac9e043842efp-1},    /* +0.14231483827328514 +0.98982144188093268 */
    /* k =  9 */ {-0x1.a9628d9c712b6p-2, 0x1.d1bb48eee2c13p-1},   /* -0.41541501300188644 +0.90963199535451833 */
    /* k = 10 */ {-0x1.aeb8c8764f0bap-1, 0x1.14cedf8bb580bp-1},   /* -0.84125353283118121 +0.54064081745559756 */
};

}  // namespace icpk
