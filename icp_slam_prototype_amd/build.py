"""Build recipe for lib/libicpk.so (hipcc, gfx950 only) -- run by
__graft_entry__.build().  hipcc cross-compiles without a GPU."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libicpk.so")

SOURCES = ["icpk_api.cpp", "icpk_sweep.cpp", "icpk_align.cpp", "icpk_batch.cpp", "icpk_frames_batch.cpp", "icpk_frontend.cpp", "icpk_comm.cpp",
           "kernels_nn.hip", "kernels_reduce.hip", "kernels_transform.hip", "kernels_backproject.hip", "kernels_sort.hip",
           "kernels_nn_pruned.hip", "kernels_loop.hip", "kernels_grid.hip", "kernels_frontend.hip",
           "icpk_map.cpp", "kernels_map.hip", "icpk_fast.cpp", "kernels_fast.hip", "kernels_map_nn.hip", "kernels_robust.hip",
           "icpk_voxel.cpp", "kernels_voxel.hip", "icpk_normals.cpp", "kernels_normals.hip",
           "icpk_filter.cpp", "kernels_filter.hip", "icpk_gicp.cpp", "kernels_gicp.hip",
           "icpk_score.cpp", "kernels_score.hip", "icpk_fpfh.cpp", "kernels_fpfh.hip", "icpk_global.cpp",
           "icpk_color.cpp", "kernels_color.hip", "icpk_posegraph.cpp", "kernels_posegraph.hip",
           "icpk_tsdf.cpp", "kernels_tsdf.hip", "icpk_bilateral.cpp", "kernels_bilateral.hip",
           "icpk_pyramid.cpp", "kernels_pyramid.hip", "icpk_projective.cpp", "kernels_projective.hip",
           "kernels_pyramid_color.hip", "icpk_raycast_color.cpp", "kernels_raycast_color.hip",
           "icpk_fern.cpp", "kernels_fern.hip", "icpk_frame_view.cpp", "kernels_frame_view.hip",
           "icpk_sdf_track.cpp", "kernels_sdf_track.hip", "icpk_tsdf_apply.cpp", "kernels_tsdf_apply.hip"]

# -ffp-contract=off: the exact kernels spell out every fma they want; nothing may
# be fused behind their back (host solve included).  No -ffast-math anywhere.
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-I", CSRC]


def _newest_src():
    paths = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    paths.append(os.path.join(ROOT, "include", "icpk.h"))
    return max(os.path.getmtime(p) for p in paths)


def build(force=False, verbose=False, extra=(), out=None):
    """out: alternative output path (diagnostic builds, e.g. tools/stamp_pruned.py)."""
    os.makedirs(LIBDIR, exist_ok=True)
    if out is None and not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest_src():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for s in SOURCES:
        o = os.path.join(LIBDIR if out is None else os.path.dirname(out), s.rsplit(".", 1)[0] + ".o")
        cmd = [hipcc] + FLAGS + list(extra) + ["-x", "hip", "-c", os.path.join(CSRC, s), "-o", o]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        objs.append(o)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out or LIB] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out or LIB


CPP_TEST = os.path.join(LIBDIR, "test_icp_align")


def build_cpp_test(force=False):
    """Host-only C++ program over icp_align.hpp + the C ABI (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_icp_align.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(CPP_TEST) and os.path.getmtime(CPP_TEST) >= newest:
        return CPP_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", CPP_TEST])
    return CPP_TEST


TRACKER_BENCH = os.path.join(LIBDIR, "tracker_bench")


def build_tracker_bench(force=False):
    """Host-only C++ program over the C ABI: the frame path timed without an interpreter (bench.py's tracker_path runs
    it as a child process)."""
    src = os.path.join(ROOT, "tests", "cpp", "tracker_bench.cpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, LIB, os.path.join(ROOT, "include", "icpk.h")))
    if not force and os.path.exists(TRACKER_BENCH) and os.path.getmtime(TRACKER_BENCH) >= newest:
        return TRACKER_BENCH
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-L", LIBDIR,
                           "-licpk", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath-link,/opt/rocm/lib", "-o", TRACKER_BENCH])
    return TRACKER_BENCH


MAP_TEST = os.path.join(LIBDIR, "test_map_tracker")


def build_map_test(force=False):
    """Host-only C++ program over icp_align.hpp's icp::Map / icp::MapTracker (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_map_tracker.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_map.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(MAP_TEST) and os.path.getmtime(MAP_TEST) >= newest:
        return MAP_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", MAP_TEST])
    return MAP_TEST


MAP_FAST_TEST = os.path.join(LIBDIR, "test_map_tracker_fast")


def build_map_fast_test(force=False):
    """Host-only C++ program over icp::MapTracker's colour overload and icp::detectFAST (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_map_tracker_fast.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_map.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(MAP_FAST_TEST) and os.path.getmtime(MAP_FAST_TEST) >= newest:
        return MAP_FAST_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", MAP_FAST_TEST])
    return MAP_FAST_TEST


MAP_DENSE_TEST = os.path.join(LIBDIR, "test_map_tracker_dense")


def build_map_dense_test(force=False):
    """Host-only C++ program over icp::MapTracker with dense = true (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_map_tracker_dense.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_map.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(MAP_DENSE_TEST) and os.path.getmtime(MAP_DENSE_TEST) >= newest:
        return MAP_DENSE_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", MAP_DENSE_TEST])
    return MAP_DENSE_TEST


VOXEL_TEST = os.path.join(LIBDIR, "test_voxel")


def build_voxel_test(force=False):
    """Host-only C++ program over icp::Engine::voxelDownsample and icp::Tracker's voxelLeaf (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_voxel.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(VOXEL_TEST) and os.path.getmtime(VOXEL_TEST) >= newest:
        return VOXEL_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", VOXEL_TEST])
    return VOXEL_TEST


NORMALS_TEST = os.path.join(LIBDIR, "test_normals")


def build_normals_test(force=False):
    """Host-only C++ program over icp::Engine::estimateTargetNormals / normalStats (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_normals.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(NORMALS_TEST) and os.path.getmtime(NORMALS_TEST) >= newest:
        return NORMALS_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", NORMALS_TEST])
    return NORMALS_TEST


FILTER_TEST = os.path.join(LIBDIR, "test_filter")


def build_filter_test(force=False):
    """Host-only C++ program over icp::Engine::removeOutliers / outlierStats and icp::Tracker's outlierFilter (g++,
    links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_filter.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(FILTER_TEST) and os.path.getmtime(FILTER_TEST) >= newest:
        return FILTER_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", FILTER_TEST])
    return FILTER_TEST


GICP_TEST = os.path.join(LIBDIR, "test_gicp")


def build_gicp_test(force=False):
    """Host-only C++ program over icp::Engine's plane-to-plane surface: estimateSourceNormals / setSourceNormals /
    sourceNormals / setPlaneToPlane (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_gicp.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(GICP_TEST) and os.path.getmtime(GICP_TEST) >= newest:
        return GICP_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", GICP_TEST])
    return GICP_TEST


COLOR_TEST = os.path.join(LIBDIR, "test_color")


def build_color_test(force=False):
    """Host-only C++ program over icp::Engine's colored ICP surface: setTargetColors / setSourceColors /
    estimateTargetColorGradients / setColored (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_color.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(COLOR_TEST) and os.path.getmtime(COLOR_TEST) >= newest:
        return COLOR_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", COLOR_TEST])
    return COLOR_TEST


SCORE_TEST = os.path.join(LIBDIR, "test_score")


def build_score_test(force=False):
    """Host-only C++ program over icp::Engine::scorePoses / scoreCurrent (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_score.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(SCORE_TEST) and os.path.getmtime(SCORE_TEST) >= newest:
        return SCORE_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", SCORE_TEST])
    return SCORE_TEST


FPFH_TEST = os.path.join(LIBDIR, "test_fpfh")


def build_fpfh_test(force=False):
    """Host-only C++ program over icp::Engine::computeFPFH / matchFeatures / registerGlobal (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_fpfh.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(FPFH_TEST) and os.path.getmtime(FPFH_TEST) >= newest:
        return FPFH_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", FPFH_TEST])
    return FPFH_TEST


POSE_GRAPH_TEST = os.path.join(LIBDIR, "test_pose_graph")


def build_pose_graph_test(force=False):
    """Host-only C++ program over icp::PoseGraph (icp_pose_graph.hpp, K18) (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_pose_graph.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_pose_graph.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(POSE_GRAPH_TEST) and os.path.getmtime(POSE_GRAPH_TEST) >= newest:
        return POSE_GRAPH_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", POSE_GRAPH_TEST])
    return POSE_GRAPH_TEST


TSDF_TEST = os.path.join(LIBDIR, "test_tsdf")


def build_tsdf_test(force=False):
    """Host-only C++ program over icp::TsdfVolume (icp_tsdf.hpp, K19) (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_tsdf.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(TSDF_TEST) and os.path.getmtime(TSDF_TEST) >= newest:
        return TSDF_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", TSDF_TEST])
    return TSDF_TEST


TSDF_RAYCAST_TEST = os.path.join(LIBDIR, "test_tsdf_raycast")


def build_tsdf_raycast_test(force=False):
    """Host-only C++ program over icp::TsdfVolume::raycast / getRaycast / raycastToTarget (icp_tsdf.hpp, K20) (g++,
    links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_tsdf_raycast.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(TSDF_RAYCAST_TEST) and os.path.getmtime(TSDF_RAYCAST_TEST) >= newest:
        return TSDF_RAYCAST_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", TSDF_RAYCAST_TEST])
    return TSDF_RAYCAST_TEST


TSDF_MESH_TEST = os.path.join(LIBDIR, "test_tsdf_mesh")


def build_tsdf_mesh_test(force=False):
    """Host-only C++ program over icp::TsdfVolume::extractMesh / getMesh / setPlanes (icp_tsdf.hpp, K21) (g++, links
    -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_tsdf_mesh.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(TSDF_MESH_TEST) and os.path.getmtime(TSDF_MESH_TEST) >= newest:
        return TSDF_MESH_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", TSDF_MESH_TEST])
    return TSDF_MESH_TEST


TSDF_SHIFT_TEST = os.path.join(LIBDIR, "test_tsdf_shift")


def build_tsdf_shift_test(force=False):
    """Host-only C++ program over icp::TsdfVolume::shift / extractLeaving / params / getBox (icp_tsdf.hpp, K23) (g++,
    links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_tsdf_shift.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(TSDF_SHIFT_TEST) and os.path.getmtime(TSDF_SHIFT_TEST) >= newest:
        return TSDF_SHIFT_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", TSDF_SHIFT_TEST])
    return TSDF_SHIFT_TEST


TSDF_REFUSE_TEST = os.path.join(LIBDIR, "test_tsdf_refuse")


def build_tsdf_refuse_test(force=False):
    """Host-only C++ program over icp::TsdfVolume::deintegrate / apply / refuse (icp_tsdf.hpp, K30) (g++, links
    -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_tsdf_refuse.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(TSDF_REFUSE_TEST) and os.path.getmtime(TSDF_REFUSE_TEST) >= newest:
        return TSDF_REFUSE_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", TSDF_REFUSE_TEST])
    return TSDF_REFUSE_TEST


TSDF_MESH_HOST_SANITIZED = os.path.join(LIBDIR, "tsdf_mesh_host_sanitized")


def build_tsdf_mesh_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/tsdf_mesh_host_main.cpp (its own main, no GPU) with icpk_tsdf.cpp --
    and so csrc/tsdf_rule.h -- compiled under -fsanitize=address,undefined on the host side; everything else icpk_tsdf.cpp
    refers to comes from libicpk.so as it is.  Run the program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "tsdf_mesh_host_main.cpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, LIB))
    if not force and os.path.exists(TSDF_MESH_HOST_SANITIZED) and os.path.getmtime(TSDF_MESH_HOST_SANITIZED) >= newest:
        return TSDF_MESH_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_tsdf.cpp"), "icpk_tsdf_sanitized.o"), (src, "tsdf_mesh_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-o", TSDF_MESH_HOST_SANITIZED])
    return TSDF_MESH_HOST_SANITIZED


TSDF_SHIFT_HOST_SANITIZED = os.path.join(LIBDIR, "tsdf_shift_host_sanitized")


def build_tsdf_shift_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/tsdf_shift_host_main.cpp (its own main, no GPU) over the host-callable
    shift rule of csrc/tsdf_rule.h (the kept box, its predicates, the origin), compiled under
    -fsanitize=address,undefined with -ffp-contract=off as the library is.  Header only: nothing is linked.  Run the
    program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "tsdf_shift_host_main.cpp")
    hdr = os.path.join(CSRC, "tsdf_rule.h")
    os.makedirs(LIBDIR, exist_ok=True)
    newest = max(os.path.getmtime(p) for p in (src, hdr))
    if not force and os.path.exists(TSDF_SHIFT_HOST_SANITIZED) and os.path.getmtime(TSDF_SHIFT_HOST_SANITIZED) >= newest:
        return TSDF_SHIFT_HOST_SANITIZED
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o",
                           TSDF_SHIFT_HOST_SANITIZED])
    return TSDF_SHIFT_HOST_SANITIZED


TSDF_APPLY_HOST_SANITIZED = os.path.join(LIBDIR, "tsdf_apply_host_sanitized")


def build_tsdf_apply_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/tsdf_apply_host_main.cpp (its own main, no GPU) with icpk_tsdf_apply.cpp
    -- the op-list validation, icpk_tsdf_voxel_apply and so the signed update rule of csrc/tsdf_rule.h -- compiled under
    -fsanitize=address,undefined on the host side; everything else icpk_tsdf_apply.cpp refers to comes from libicpk.so as
    it is.  Run the program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "tsdf_apply_host_main.cpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, LIB))
    if not force and os.path.exists(TSDF_APPLY_HOST_SANITIZED) and os.path.getmtime(TSDF_APPLY_HOST_SANITIZED) >= newest:
        return TSDF_APPLY_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_tsdf_apply.cpp"), "icpk_tsdf_apply_sanitized.o"), (src, "tsdf_apply_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-o", TSDF_APPLY_HOST_SANITIZED])
    return TSDF_APPLY_HOST_SANITIZED


BILATERAL_TEST = os.path.join(LIBDIR, "test_bilateral")


def build_bilateral_test(force=False):
    """Host-only C++ program over icp::Engine::bilateralDepthImage / backprojectSmoothed (icp_align.hpp, K22) (g++, links
    -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_bilateral.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(BILATERAL_TEST) and os.path.getmtime(BILATERAL_TEST) >= newest:
        return BILATERAL_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", BILATERAL_TEST])
    return BILATERAL_TEST


BILATERAL_HOST_SANITIZED = os.path.join(LIBDIR, "bilateral_host_sanitized")


def build_bilateral_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/bilateral_host_main.cpp (its own main, no GPU) with icpk_bilateral.cpp
    -- and so csrc/bilateral_rule.h -- compiled under -fsanitize=address,undefined on the host side.  icpk_bilateral.cpp
    is host only and refers to nothing else of the library, so the program does not link it.  Run the program it returns
    directly."""
    src = os.path.join(ROOT, "tests", "cpp", "bilateral_host_main.cpp")
    deps = [src, os.path.join(CSRC, "icpk_bilateral.cpp"), os.path.join(CSRC, "bilateral_rule.h"),
            os.path.join(ROOT, "include", "icpk.h")]
    os.makedirs(LIBDIR, exist_ok=True)
    if not force and os.path.exists(BILATERAL_HOST_SANITIZED) and \
            os.path.getmtime(BILATERAL_HOST_SANITIZED) >= max(os.path.getmtime(p) for p in deps):
        return BILATERAL_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_bilateral.cpp"), "icpk_bilateral_sanitized.o"), (src, "bilateral_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-o", BILATERAL_HOST_SANITIZED])
    return BILATERAL_HOST_SANITIZED


PYRAMID_TEST = os.path.join(LIBDIR, "test_pyramid")


def build_pyramid_test(force=False):
    """Host-only C++ program over icp::Engine::buildDepthPyramid / depthPyramidLevel / backprojectPyramidLevel
    (icp_align.hpp, K24) (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_pyramid.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(PYRAMID_TEST) and os.path.getmtime(PYRAMID_TEST) >= newest:
        return PYRAMID_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", PYRAMID_TEST])
    return PYRAMID_TEST


PYRAMID_HOST_SANITIZED = os.path.join(LIBDIR, "pyramid_host_sanitized")


def build_pyramid_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/pyramid_host_main.cpp (its own main, no GPU) with icpk_pyramid.cpp --
    and so csrc/pyramid_rule.h -- compiled under -fsanitize=address,undefined on the host side.  icpk_pyramid.cpp is
    host only and refers to nothing else of the library, so the program does not link it.  Run the program it returns
    directly."""
    src = os.path.join(ROOT, "tests", "cpp", "pyramid_host_main.cpp")
    deps = [src, os.path.join(CSRC, "icpk_pyramid.cpp"), os.path.join(CSRC, "pyramid_rule.h"),
            os.path.join(ROOT, "include", "icpk.h")]
    os.makedirs(LIBDIR, exist_ok=True)
    if not force and os.path.exists(PYRAMID_HOST_SANITIZED) and \
            os.path.getmtime(PYRAMID_HOST_SANITIZED) >= max(os.path.getmtime(p) for p in deps):
        return PYRAMID_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_pyramid.cpp"), "icpk_pyramid_sanitized.o"), (src, "pyramid_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-o", PYRAMID_HOST_SANITIZED])
    return PYRAMID_HOST_SANITIZED


PROJECTIVE_TEST = os.path.join(LIBDIR, "test_projective")


def build_projective_test(force=False):
    """Host-only C++ program over icp::TsdfVolume::alignProjective / projectiveAssociate / projectiveTrace (icp_tsdf.hpp,
    K25) (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_projective.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(PROJECTIVE_TEST) and os.path.getmtime(PROJECTIVE_TEST) >= newest:
        return PROJECTIVE_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", PROJECTIVE_TEST])
    return PROJECTIVE_TEST


FRAME_ODOMETRY_TEST = os.path.join(LIBDIR, "test_frame_odometry")


def build_frame_odometry_test(force=False):
    """Host-only C++ program over icp::Engine::buildFrameView / setProjectiveView and icp::FrameOdometry (icp_align.hpp,
    icp_odometry.hpp, K28) (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_frame_odometry.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_odometry.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(FRAME_ODOMETRY_TEST) and os.path.getmtime(FRAME_ODOMETRY_TEST) >= newest:
        return FRAME_ODOMETRY_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", FRAME_ODOMETRY_TEST])
    return FRAME_ODOMETRY_TEST


SDF_TRACK_TEST = os.path.join(LIBDIR, "test_sdf_track")


def build_sdf_track_test(force=False):
    """Host-only C++ program over icp::TsdfVolume::alignSdf / sdfReduce / sdfAssociate / sdfTrace (icp_tsdf.hpp, K29) (g++,
    links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_sdf_track.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(SDF_TRACK_TEST) and os.path.getmtime(SDF_TRACK_TEST) >= newest:
        return SDF_TRACK_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", SDF_TRACK_TEST])
    return SDF_TRACK_TEST


SDF_TRACK_HOST_SANITIZED = os.path.join(LIBDIR, "sdf_track_host_sanitized")


def build_sdf_track_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/sdf_track_host_main.cpp (its own main, no GPU) with icpk_sdf_track.cpp
    -- and so csrc/sdf_track_rule.h, projective_rule.h and tsdf_rule.h -- compiled under -fsanitize=address,undefined on
    the host side; everything else icpk_sdf_track.cpp refers to (the volume's accessor, the launchers its device entry
    points call) comes from libicpk.so as it is.  The program calls the host-only entry point alone, every array
    allocated at exactly its size.  Run the program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "sdf_track_host_main.cpp")
    build()
    deps = [src, LIB, os.path.join(CSRC, "icpk_sdf_track.cpp")] + \
        [os.path.join(CSRC, h) for h in ("sdf_track_rule.h", "projective_rule.h", "tsdf_rule.h")]
    if not force and os.path.exists(SDF_TRACK_HOST_SANITIZED) and \
            os.path.getmtime(SDF_TRACK_HOST_SANITIZED) >= max(os.path.getmtime(p) for p in deps):
        return SDF_TRACK_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_sdf_track.cpp"), "icpk_sdf_track_sanitized.o"), (src, "sdf_track_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-o", SDF_TRACK_HOST_SANITIZED])
    return SDF_TRACK_HOST_SANITIZED


PROJECTIVE_HOST_SANITIZED = os.path.join(LIBDIR, "projective_host_sanitized")


def build_projective_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/projective_host_main.cpp (its own main, no GPU) with icpk_projective.cpp
    -- and so csrc/projective_rule.h -- compiled under -fsanitize=address,undefined on the host side; everything else
    icpk_projective.cpp refers to (the pose inversion, the launchers its device entry points call) comes from libicpk.so
    as it is.  The program calls the host-only entry point alone.  Run the program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "projective_host_main.cpp")
    build()
    deps = [src, LIB, os.path.join(CSRC, "icpk_projective.cpp"), os.path.join(CSRC, "projective_rule.h")]
    if not force and os.path.exists(PROJECTIVE_HOST_SANITIZED) and \
            os.path.getmtime(PROJECTIVE_HOST_SANITIZED) >= max(os.path.getmtime(p) for p in deps):
        return PROJECTIVE_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_projective.cpp"), "icpk_projective_sanitized.o"), (src, "projective_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-o", PROJECTIVE_HOST_SANITIZED])
    return PROJECTIVE_HOST_SANITIZED


PROJECTIVE_COLOR_TEST = os.path.join(LIBDIR, "test_projective_color")


def build_projective_color_test(force=False):
    """Host-only C++ program over icp::Engine::setPyramidIntensity and icp::TsdfVolume::raycastColorGradients /
    alignProjectiveColored (icp_align.hpp, icp_tsdf.hpp, K26) (g++, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_projective_color.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(PROJECTIVE_COLOR_TEST) and os.path.getmtime(PROJECTIVE_COLOR_TEST) >= newest:
        return PROJECTIVE_COLOR_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", PROJECTIVE_COLOR_TEST])
    return PROJECTIVE_COLOR_TEST


PROJECTIVE_COLOR_HOST_SANITIZED = os.path.join(LIBDIR, "projective_color_host_sanitized")


def build_projective_color_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/projective_color_host_main.cpp (its own main, no GPU) with
    icpk_pyramid.cpp, icpk_raycast_color.cpp and icpk_projective.cpp -- and so csrc/pyramid_rule.h, raycast_color_rule.h
    and projective_rule.h -- compiled under -fsanitize=address,undefined on the host side; everything else
    icpk_projective.cpp refers to (the pose inversion, the launchers its device entry points call) comes from libicpk.so
    as it is.  The program calls the three host-only entry points of K26 alone.  Run the program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "projective_color_host_main.cpp")
    build()
    host = ["icpk_pyramid.cpp", "icpk_raycast_color.cpp", "icpk_projective.cpp"]
    deps = [src, LIB] + [os.path.join(CSRC, f) for f in host + ["pyramid_rule.h", "raycast_color_rule.h", "projective_rule.h"]]
    if not force and os.path.exists(PROJECTIVE_COLOR_HOST_SANITIZED) and \
            os.path.getmtime(PROJECTIVE_COLOR_HOST_SANITIZED) >= max(os.path.getmtime(p) for p in deps):
        return PROJECTIVE_COLOR_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in [(os.path.join(CSRC, f), f.rsplit(".", 1)[0] + "_color_sanitized.o") for f in host] + \
            [(src, "projective_color_host_main.o")]:
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-o", PROJECTIVE_COLOR_HOST_SANITIZED])
    return PROJECTIVE_COLOR_HOST_SANITIZED


FERN_TEST = os.path.join(LIBDIR, "test_fern")


def build_fern_test(force=False):
    """Host-only C++ program over icp::FernDatabase and icp::TsdfVolume::relocalise (icp_tsdf.hpp, K27) (g++, links
    -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_fern.cpp")
    hdrs = [os.path.join(HERE, "include", h) for h in ("icp_align.hpp", "icp_tsdf.hpp")]
    build()
    newest = max(os.path.getmtime(p) for p in [src, LIB] + hdrs)
    if not force and os.path.exists(FERN_TEST) and os.path.getmtime(FERN_TEST) >= newest:
        return FERN_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", FERN_TEST])
    return FERN_TEST


FERN_HOST_SANITIZED = os.path.join(LIBDIR, "fern_host_sanitized")


def build_fern_host_sanitized(force=False):
    """DIAGNOSTIC, not part of build(): tests/cpp/fern_host_main.cpp (its own main, no GPU) with icpk_fern.cpp -- and so
    csrc/fern_rule.h -- compiled under -fsanitize=address,undefined on the host side; everything else icpk_fern.cpp
    refers to (the launchers its device entry points call) comes from libicpk.so as it is.  The program calls the three
    host-only entry points alone.  Run the program it returns directly."""
    src = os.path.join(ROOT, "tests", "cpp", "fern_host_main.cpp")
    build()
    deps = [src, LIB, os.path.join(CSRC, "icpk_fern.cpp"), os.path.join(CSRC, "fern_rule.h")]
    if not force and os.path.exists(FERN_HOST_SANITIZED) and \
            os.path.getmtime(FERN_HOST_SANITIZED) >= max(os.path.getmtime(p) for p in deps):
        return FERN_HOST_SANITIZED
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    objs = []
    for path, name in ((os.path.join(CSRC, "icpk_fern.cpp"), "icpk_fern_sanitized.o"), (src, "fern_host_main.o")):
        objs.append(os.path.join(LIBDIR, name))
        subprocess.check_call([hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", objs[-1]])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                          ["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-o", FERN_HOST_SANITIZED])
    return FERN_HOST_SANITIZED


THREADS_TEST = os.path.join(LIBDIR, "test_threads")


def build_threads_test(force=False):
    """Host-only C++ program: one icp::Engine + icp::Tracker per std::thread against the same sequences one after the
    other (g++ -pthread, links -licpk)."""
    src = os.path.join(ROOT, "tests", "cpp", "test_threads.cpp")
    hdr = os.path.join(HERE, "include", "icp_align.hpp")
    build()
    newest = max(os.path.getmtime(p) for p in (src, hdr, LIB))
    if not force and os.path.exists(THREADS_TEST) and os.path.getmtime(THREADS_TEST) >= newest:
        return THREADS_TEST
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(HERE, "include"), src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", THREADS_TEST])
    return THREADS_TEST


FAKE_RCCL = os.path.join(LIBDIR, "libfake_rccl.so")


def build_fake_rccl(force=False):
    """TEST INFRASTRUCTURE: tests/cpp/fake_rccl.cpp (collectives over shared memory for ranks that share
    one GPU), loaded through ICPK_RCCL_LIB by tests/test_gpu_comm_two_ranks.py only."""
    src = os.path.join(ROOT, "tests", "cpp", "fake_rccl.cpp")
    os.makedirs(LIBDIR, exist_ok=True)
    if not force and os.path.exists(FAKE_RCCL) and os.path.getmtime(FAKE_RCCL) >= os.path.getmtime(src):
        return FAKE_RCCL
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip", "--offload-arch=gfx950", src, "-o",
                           FAKE_RCCL, "-lrt"])
    return FAKE_RCCL


SOLVE_PROBE = os.path.join(LIBDIR, "libsolve_probe.so")


def build_solve_probe(force=False):
    """TEST INFRASTRUCTURE: tests/cpp/solve_probe.hip (csrc/solve_impl.h run over arrays of cases on the device and
    on the host), loaded by tests/test_gpu_solve_device.py and tests/test_solve_probe_host.py only.  Compiled with
    exactly FLAGS, so its device and host code are generated as they are for libicpk.so."""
    src = os.path.join(ROOT, "tests", "cpp", "solve_probe.hip")
    os.makedirs(LIBDIR, exist_ok=True)
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(CSRC, "solve_impl.h"), os.path.abspath(__file__)))
    if not force and os.path.exists(SOLVE_PROBE) and os.path.getmtime(SOLVE_PROBE) >= newest:
        return SOLVE_PROBE
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-shared", "-x", "hip", src, "-o", SOLVE_PROBE])
    return SOLVE_PROBE


SCAN_PROBE = os.path.join(LIBDIR, "libscan_probe.so")


def build_scan_probe(force=False):
    """TEST INFRASTRUCTURE: tests/cpp/scan_probe.hip (csrc/block_scan.h run by one workgroup over host arrays), loaded by
    tests/test_gpu_scan_probe.py only.  Compiled with exactly FLAGS, so its device code is generated as it is for
    libicpk.so."""
    src = os.path.join(ROOT, "tests", "cpp", "scan_probe.hip")
    os.makedirs(LIBDIR, exist_ok=True)
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(CSRC, "block_scan.h"), os.path.abspath(__file__)))
    if not force and os.path.exists(SCAN_PROBE) and os.path.getmtime(SCAN_PROBE) >= newest:
        return SCAN_PROBE
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + ["-shared", "-x", "hip", src, "-o", SCAN_PROBE])
    return SCAN_PROBE


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_cpp_test(force="--force" in sys.argv))
    print(build_tracker_bench(force="--force" in sys.argv))
    print(build_map_test(force="--force" in sys.argv))
    print(build_map_fast_test(force="--force" in sys.argv))
    print(build_map_dense_test(force="--force" in sys.argv))
    print(build_voxel_test(force="--force" in sys.argv))
    print(build_normals_test(force="--force" in sys.argv))
    print(build_filter_test(force="--force" in sys.argv))
    print(build_gicp_test(force="--force" in sys.argv))
    print(build_color_test(force="--force" in sys.argv))
    print(build_score_test(force="--force" in sys.argv))
    print(build_fpfh_test(force="--force" in sys.argv))
    print(build_pose_graph_test(force="--force" in sys.argv))
    print(build_tsdf_test(force="--force" in sys.argv))
    print(build_tsdf_raycast_test(force="--force" in sys.argv))
    print(build_tsdf_mesh_test(force="--force" in sys.argv))
    print(build_tsdf_shift_test(force="--force" in sys.argv))
    print(build_tsdf_refuse_test(force="--force" in sys.argv))
    print(build_bilateral_test(force="--force" in sys.argv))
    print(build_pyramid_test(force="--force" in sys.argv))
    print(build_projective_test(force="--force" in sys.argv))
    print(build_projective_color_test(force="--force" in sys.argv))
    print(build_fern_test(force="--force" in sys.argv))
    print(build_frame_odometry_test(force="--force" in sys.argv))
    print(build_sdf_track_test(force="--force" in sys.argv))
    print(build_threads_test(force="--force" in sys.argv))
