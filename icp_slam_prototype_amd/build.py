"""Build recipe for lib/libicpk.so (hipcc, gfx950 only) -- run by
__graft_entry__.build().  hipcc cross-compiles without a GPU."""
import collections
import functools
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
           "icpk_sdf_track.cpp", "kernels_sdf_track.hip", "icpk_tsdf_apply.cpp", "kernels_tsdf_apply.hip",
           "icpk_esdf.cpp", "kernels_esdf.hip", "icpk_brief.cpp", "kernels_brief.hip",
           "icpk_cluster.cpp", "kernels_cluster.hip", "icpk_plane.cpp", "kernels_plane.hip"]

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


# ---- the test programs: one table row each, one builder for all of them ----------------------------------------------
# A key is the output's base name under lib/ (the three shared objects without "lib" and ".so").  A row carries its
# kind, what differs from the kind's recipe, and a doc.  The kinds:
#   mirror            g++ over tests/cpp/<key>.cpp, a host-only C++ program over the C ABI; links -licpk.
#                     Options: pthread; package_include=False (no -I of the package's include/).
#   sanitized         DIAGNOSTIC, not in DEFAULT: tests/cpp/<key minus "_sanitized">_main.cpp (its own main, no GPU) and
#                     the csrc sources of the row, compiled by hipcc under -fsanitize=address,undefined on the host side.
#                     Whatever else those sources refer to comes from libicpk.so as it is, unless links_lib=False.
#                     object_suffix names the csrc objects; two rows must never write one .o.  Run the program
#                     directly (tests/test_sanitized_programs_host.py does).
#   sanitized_header  DIAGNOSTIC, not in DEFAULT: the same for a main over csrc headers alone; g++, nothing linked.
#   probe             TEST INFRASTRUCTURE: tests/cpp/<key>.hip as a shared object compiled with exactly FLAGS, so its
#                     device and host code are generated as they are for libicpk.so.
#   fake_rccl         TEST INFRASTRUCTURE, a recipe of its own.
def _mirror(doc, **options):
    return dict(kind="mirror", doc=doc, **options)


def _sanitized(csrc, doc, **options):
    return dict(kind="sanitized", csrc=csrc, doc=doc, **options)


PROGRAMS = {
    "test_icp_align": _mirror("icp_align.hpp + the C ABI"),
    "tracker_bench": _mirror("the C ABI alone: the frame path timed without an interpreter (bench.py's tracker_path runs "
                             "it as a child process)", package_include=False),
    "test_map_tracker": _mirror("icp_align.hpp's icp::Map / icp::MapTracker (icp_map.hpp)"),
    "test_map_tracker_fast": _mirror("icp::MapTracker's colour overload and icp::detectFAST"),
    "test_map_tracker_dense": _mirror("icp::MapTracker with dense = true (K9)"),
    "test_voxel": _mirror("icp::Engine::voxelDownsample and icp::Tracker's voxelLeaf (K11)"),
    "test_normals": _mirror("icp::Engine::estimateTargetNormals / normalStats (K12)"),
    "test_filter": _mirror("icp::Engine::removeOutliers / outlierStats and icp::Tracker's outlierFilter (K13)"),
    "test_gicp": _mirror("icp::Engine's plane-to-plane surface: estimateSourceNormals / setSourceNormals / sourceNormals "
                         "/ setPlaneToPlane (K14)"),
    "test_color": _mirror("icp::Engine's colored ICP surface: setTargetColors / setSourceColors / "
                          "estimateTargetColorGradients / setColored (K17)"),
    "test_score": _mirror("icp::Engine::scorePoses / scoreCurrent (K15)"),
    "test_fpfh": _mirror("icp::Engine::computeFPFH / matchFeatures / registerGlobal (K16)"),
    "test_pose_graph": _mirror("icp::PoseGraph (icp_pose_graph.hpp, K18)"),
    "test_tsdf": _mirror("icp::TsdfVolume (icp_tsdf.hpp, K19)"),
    "test_tsdf_raycast": _mirror("icp::TsdfVolume::raycast / getRaycast / raycastToTarget (icp_tsdf.hpp, K20)"),
    "test_tsdf_mesh": _mirror("icp::TsdfVolume::extractMesh / getMesh / setPlanes (icp_tsdf.hpp, K21)"),
    "test_tsdf_shift": _mirror("icp::TsdfVolume::shift / extractLeaving / params / getBox (icp_tsdf.hpp, K23)"),
    "test_tsdf_refuse": _mirror("icp::TsdfVolume::deintegrate / apply / refuse (icp_tsdf.hpp, K30)"),
    "test_bilateral": _mirror("icp::Engine::bilateralDepthImage / backprojectSmoothed (icp_align.hpp, K22)"),
    "test_pyramid": _mirror("icp::Engine::buildDepthPyramid / depthPyramidLevel / backprojectPyramidLevel (icp_align.hpp, "
                            "K24)"),
    "test_projective": _mirror("icp::TsdfVolume::alignProjective / projectiveAssociate / projectiveTrace (icp_tsdf.hpp, "
                               "K25)"),
    "test_projective_color": _mirror("icp::Engine::setPyramidIntensity and icp::TsdfVolume::raycastColorGradients / "
                                     "alignProjectiveColored (icp_align.hpp, icp_tsdf.hpp, K26)"),
    "test_fern": _mirror("icp::FernDatabase and icp::TsdfVolume::relocalise (icp_tsdf.hpp, K27)"),
    "test_frame_odometry": _mirror("icp::Engine::buildFrameView / setProjectiveView and icp::FrameOdometry (icp_align.hpp, "
                                   "icp_odometry.hpp, K28)"),
    "test_sdf_track": _mirror("icp::TsdfVolume::alignSdf / sdfReduce / sdfAssociate / sdfTrace (icp_tsdf.hpp, K29)"),
    "test_threads": _mirror("one icp::Engine + icp::Tracker per std::thread against the same sequences one after the "
                            "other", pthread=True),
    "tsdf_mesh_host_sanitized": _sanitized(["icpk_tsdf.cpp"], "icpk_tsdf.cpp and so csrc/tsdf_rule.h"),
    "tsdf_shift_host_sanitized": dict(kind="sanitized_header", doc="the host-callable shift rule of csrc/tsdf_rule.h "
                                      "(the kept box, its predicates, the origin), with -ffp-contract=off as the library is"),
    "tsdf_apply_host_sanitized": _sanitized(["icpk_tsdf_apply.cpp"], "icpk_tsdf_apply.cpp: the op-list validation, "
                                            "icpk_tsdf_voxel_apply and so the signed update rule of csrc/tsdf_rule.h"),
    "bilateral_host_sanitized": _sanitized(["icpk_bilateral.cpp"], "icpk_bilateral.cpp and so csrc/bilateral_rule.h; it "
                                           "is host only and refers to nothing else of the library", links_lib=False),
    "pyramid_host_sanitized": _sanitized(["icpk_pyramid.cpp"], "icpk_pyramid.cpp and so csrc/pyramid_rule.h; it is host "
                                         "only and refers to nothing else of the library", links_lib=False),
    "projective_host_sanitized": _sanitized(["icpk_projective.cpp"], "icpk_projective.cpp and so csrc/projective_rule.h; "
                                            "the pose inversion and the launchers come from the library; the program "
                                            "calls the host-only entry point alone"),
    "projective_color_host_sanitized": _sanitized(
        ["icpk_pyramid.cpp", "icpk_raycast_color.cpp", "icpk_projective.cpp"], "the three host-only entry points of K26 "
        "alone, and so csrc/pyramid_rule.h, raycast_color_rule.h and projective_rule.h; the pose inversion and the "
        "launchers come from the library", object_suffix="_color_sanitized.o"),
    "fern_host_sanitized": _sanitized(["icpk_fern.cpp"], "icpk_fern.cpp and so csrc/fern_rule.h; the launchers come from "
                                      "the library; the program calls the three host-only entry points alone"),
    "sdf_track_host_sanitized": _sanitized(["icpk_sdf_track.cpp"], "icpk_sdf_track.cpp and so csrc/sdf_track_rule.h, "
                                           "projective_rule.h and tsdf_rule.h; the volume's accessor and the launchers "
                                           "come from the library; the program calls the host-only entry point alone, "
                                           "every array allocated at exactly its size"),
    "fake_rccl": dict(kind="fake_rccl", doc="tests/cpp/fake_rccl.cpp: collectives over shared memory for ranks that share "
                      "one GPU, loaded through ICPK_RCCL_LIB by tests/test_gpu_comm_two_ranks.py only"),
    "solve_probe": dict(kind="probe", doc="csrc/solve_impl.h run over arrays of cases on the device and on the host, "
                        "loaded by tests/test_gpu_solve_device.py and tests/test_solve_probe_host.py only"),
    "scan_probe": dict(kind="probe", doc="csrc/block_scan.h run by one workgroup over host arrays, loaded by "
                       "tests/test_gpu_scan_probe.py only"),
}

# What __graft_entry__.build() builds, in this order: everything but the sanitized diagnostics.
DEFAULT = [name for name, row in PROGRAMS.items() if not row["kind"].startswith("sanitized")]

# The rows added since the tests pinned PROGRAMS and DEFAULT as they stand (tests/test_build_recipes_host.py,
# tests/test_sanitized_programs_host.py): the same shape, the same kinds, resolved by the same plan() and program().
LATER_PROGRAMS = {
    "test_tsdf_esdf": _mirror("icp::TsdfVolume::computeEsdf / esdfPlanes / esdfBox / queryEsdf (icp_tsdf.hpp, K31)"),
    "esdf_host_sanitized": _sanitized(["icpk_esdf.cpp"], "icpk_esdf.cpp and so csrc/esdf_rule.h and tsdf_rule.h; the "
                                      "volume's refusals and the launchers come from the library; the program calls the two "
                                      "host-only entry points alone, every array allocated at exactly its size"),
    "test_brief": _mirror("icp::Engine::describeKeypoints / describePoints / describedToCloud / matchDescriptors "
                          "(icp_align.hpp, K32)"),
    "brief_host_sanitized": _sanitized(["icpk_brief.cpp"], "icpk_brief.cpp and so csrc/brief_rule.h and brief_table.h; the "
                                       "slots' plumbing and the launchers come from the library; the program calls the two "
                                       "host-only entry points alone, every array allocated at exactly its size"),
    "test_cluster": _mirror("icp::Engine::clusterDbscan / clusters (icp_align.hpp, K33)"),
    "cluster_host_sanitized": _sanitized(["icpk_cluster.cpp"], "icpk_cluster.cpp and so csrc/cluster_rule.h; the context's "
                                         "plumbing and the launchers come from the library; the program calls the host-only "
                                         "entry point alone, every array allocated at exactly its size"),
    "test_plane": _mirror("icp::Engine::segmentPlanes / planes (icp_align.hpp, K34)"),
    "plane_host_sanitized": _sanitized(["icpk_plane.cpp"], "icpk_plane.cpp and so csrc/plane_rule.h; the context's plumbing "
                                       "and the launchers come from the library; the program calls the host-only entry "
                                       "points alone, every array allocated at exactly its size"),
}

# What __graft_entry__.build() builds after DEFAULT: the later rows but the sanitized diagnostics.
LATER_DEFAULT = [name for name, row in LATER_PROGRAMS.items() if not row["kind"].startswith("sanitized")]

Plan = collections.namedtuple("Plan", "out sources deps commands links_lib")


def plan(name):
    """How PROGRAMS[name] (or LATER_PROGRAMS[name]) is built: its output, the sources its row names, what it is rebuilt
    after (one rule per kind) and the compiler commands.  Runs nothing."""
    row = PROGRAMS[name] if name in PROGRAMS else LATER_PROGRAMS[name]
    kind = row["kind"]
    cpp = os.path.join(ROOT, "tests", "cpp")
    abi = os.path.join(ROOT, "include", "icpk.h")
    rules = [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")]
    shared = kind in ("probe", "fake_rccl")
    out = os.path.join(LIBDIR, "lib" + name + ".so" if shared else name)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if kind == "mirror":
        src = os.path.join(cpp, name + ".cpp")
        mirrors = os.path.join(HERE, "include")
        deps = [src, LIB, abi] + [os.path.join(mirrors, h) for h in sorted(os.listdir(mirrors)) if h.endswith(".hpp")]
        cmd = ["g++", "-std=c++17", "-O2", "-Wall"] + (["-pthread"] if row.get("pthread") else []) + \
            ["-I", os.path.join(ROOT, "include")] + (["-I", mirrors] if row.get("package_include", True) else []) + \
            [src, "-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath-link,/opt/rocm/lib", "-o", out]
        return Plan(out, [src], deps, [cmd], True)
    if kind == "sanitized":
        main = os.path.join(cpp, name[:-len("_sanitized")] + "_main.cpp")
        links = row.get("links_lib", True)
        units = [(os.path.join(CSRC, f), f.rsplit(".", 1)[0] + row.get("object_suffix", "_sanitized.o")) for f in row["csrc"]]
        units.append((main, os.path.basename(main)[:-len(".cpp")] + ".o"))
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
        objs = [os.path.join(LIBDIR, o) for _, o in units]
        cmds = [[hipcc] + FLAGS + san + ["-x", "hip", "-c", path, "-o", o] for (path, _), o in zip(units, objs)]
        cmds.append([hipcc, "--offload-arch=gfx950", "-fsanitize=address,undefined"] + objs +
                    (["-L", LIBDIR, "-licpk", "-Wl,-rpath,$ORIGIN"] if links else []) + ["-o", out])
        sources = [path for path, _ in units]
        return Plan(out, sources, sources + rules + [abi] + ([LIB] if links else []), cmds, links)
    if kind == "sanitized_header":
        src = os.path.join(cpp, name[:-len("_sanitized")] + "_main.cpp")
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-omit-frame-pointer",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", out]
        return Plan(out, [src], [src] + rules, [cmd], False)
    if kind == "probe":
        src = os.path.join(cpp, name + ".hip")
        cmd = [hipcc] + FLAGS + ["-shared", "-x", "hip", src, "-o", out]
        return Plan(out, [src], [src] + rules + [os.path.abspath(__file__)], [cmd], False)
    assert kind == "fake_rccl", kind
    src = os.path.join(cpp, name + ".cpp")
    cmd = [hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip", "--offload-arch=gfx950", src, "-o", out, "-lrt"]
    return Plan(out, [src], [src], [cmd], False)


def program(name, force=False):
    """Build PROGRAMS[name] (or LATER_PROGRAMS[name]) if it is older than anything plan(name) says it depends on; returns its path under lib/."""
    p = plan(name)
    os.makedirs(LIBDIR, exist_ok=True)
    if p.links_lib:
        build()
    if force or not os.path.exists(p.out) or os.path.getmtime(p.out) < max(os.path.getmtime(d) for d in p.deps):
        for cmd in p.commands:
            subprocess.check_call(cmd)
    return p.out


TRACKER_BENCH = os.path.join(LIBDIR, "tracker_bench")  # bench.py's tracker_path looks here before it builds


def build_tracker_bench(force=False):
    return program("tracker_bench", force)


# The builders' names from before the table, frozen: a caller written against the old interface -- the tests as they
# stood before this table, which every later build is still held to -- keeps working.  This is the whole list: a new
# row gets no such name, and new code calls program().
_FORMER_NAMES = {
    "build_cpp_test": "test_icp_align", "build_map_test": "test_map_tracker", "build_map_fast_test": "test_map_tracker_fast",
    "build_map_dense_test": "test_map_tracker_dense", "build_voxel_test": "test_voxel", "build_normals_test": "test_normals",
    "build_filter_test": "test_filter", "build_gicp_test": "test_gicp", "build_color_test": "test_color",
    "build_score_test": "test_score", "build_fpfh_test": "test_fpfh", "build_pose_graph_test": "test_pose_graph",
    "build_tsdf_test": "test_tsdf", "build_tsdf_raycast_test": "test_tsdf_raycast", "build_tsdf_mesh_test": "test_tsdf_mesh",
    "build_tsdf_shift_test": "test_tsdf_shift", "build_tsdf_refuse_test": "test_tsdf_refuse",
    "build_bilateral_test": "test_bilateral", "build_pyramid_test": "test_pyramid", "build_projective_test": "test_projective",
    "build_projective_color_test": "test_projective_color", "build_fern_test": "test_fern",
    "build_frame_odometry_test": "test_frame_odometry", "build_sdf_track_test": "test_sdf_track",
    "build_threads_test": "test_threads", "build_tsdf_mesh_host_sanitized": "tsdf_mesh_host_sanitized",
    "build_tsdf_shift_host_sanitized": "tsdf_shift_host_sanitized", "build_tsdf_apply_host_sanitized": "tsdf_apply_host_sanitized",
    "build_bilateral_host_sanitized": "bilateral_host_sanitized", "build_pyramid_host_sanitized": "pyramid_host_sanitized",
    "build_projective_host_sanitized": "projective_host_sanitized",
    "build_projective_color_host_sanitized": "projective_color_host_sanitized", "build_fern_host_sanitized": "fern_host_sanitized",
    "build_sdf_track_host_sanitized": "sdf_track_host_sanitized", "build_fake_rccl": "fake_rccl",
    "build_solve_probe": "solve_probe", "build_scan_probe": "scan_probe",
}
globals().update({former: functools.partial(program, name) for former, name in _FORMER_NAMES.items()})


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    for name in DEFAULT + LATER_DEFAULT:
        print(program(name, force="--force" in sys.argv))
