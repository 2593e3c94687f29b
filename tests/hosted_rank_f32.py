"""One rank of a HOSTED multi-process solve of an AVS_PRECISION_F32 context on float vectors
(tests/test_gpu_dist_f32.py::test_processes_direct_transport_float_vectors).

As tests/hosted_rank.py (whose blob hand-over through files it reuses), with a float context and AVS_DIST_F32_VECTORS=1 in the
environment: both processes use cuda:0, map each other's comm block through HIP IPC handles and run the direct transport's float loop."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hosted_rank import wait_for  # noqa: E402


def main():
    workdir, rank, world, scene, tol = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], float(sys.argv[5])
    import torch
    from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes
    dev = torch.device("cuda:0")
    sc = {"beam": lambda: scenes.fat_beam(64, 3, device=dev),
          "beam128L4_brick": lambda: scenes.fat_beam(128, 4, device=dev)}[scene]()   # (AVS_BRICK=1 in the environment)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    pi = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pi.levels, precision=capi.PRECISION_F32)
    pp.apply(s)
    s.set_scene_fields(sc)
    capi.check(s.lib.avs_dist_init_hosted(s.h, rank, world))
    s.dist_assemble()
    blob = (C.c_uint8 * capi.DIST_BLOB_BYTES)()
    capi.check(s.lib.avs_dist_export_blob(s.h, blob))
    tmp = os.path.join(workdir, f"blob_{rank}.tmp")
    open(tmp, "wb").write(bytes(blob))
    os.rename(tmp, os.path.join(workdir, f"blob_{rank}.bin"))
    allb = b""
    for q in range(world):
        wait_for(os.path.join(workdir, f"blob_{q}.bin"))
        allb += open(os.path.join(workdir, f"blob_{q}.bin"), "rb").read()
    buf = (C.c_uint8 * len(allb)).from_buffer_copy(allb)
    capi.check(s.lib.avs_dist_import_blobs(s.h, buf))    # connects the comm blocks and runs the transport self-test
    runs, xs = [], []
    for _ in range(2):                                   # twice: the second solve replays the captured graph
        info = s.dist_solve(tol, 5000)
        runs.append((info.iterations, info.converged))
        xs.append(s.dist_solution())                     # hosted group: owned entries, zeros elsewhere
    ci = s.dist_comm_info()
    fmt = s.matrix_format()
    np.save(os.path.join(workdir, f"x_{rank}.npy"), xs[0])
    np.save(os.path.join(workdir, f"x2_{rank}.npy"), xs[1])
    np.save(os.path.join(workdir, f"info_{rank}.npy"), np.array([runs[0][0], runs[0][1], runs[1][0], runs[1][1],
                                                                  s.plan_sizes.n_own, s.plan_sizes.n_halo,
                                                                  1 if ci["transport"] == "direct" else 0, ci["rccl_calls_per_iteration"],
                                                                  ci["selftest_rounds"], ci["selftest_bad_entries"],
                                                                  fmt.float_vectors, fmt.brick_tiles], np.float64))
    # keep the comm block alive until every rank has finished (a peer may still be reading its own copy of the flags)
    open(os.path.join(workdir, f"done_{rank}"), "w").write("ok")
    for q in range(world):
        wait_for(os.path.join(workdir, f"done_{q}"))
    s.close()


if __name__ == "__main__":
    main()
