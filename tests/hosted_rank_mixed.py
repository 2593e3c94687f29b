"""One rank of a HOSTED multi-process solve of an fp64 context with AVS_DIST_MIXED_PRECISION in the environment
(tests/test_gpu_dist_mixed.py::test_processes_direct_transport).

As tests/hosted_rank_f32.py (blobs handed over through files, both processes on cuda:0, comm blocks mapped through HIP IPC handles): the
direct transport's loop at `tol` twice -- the second solve replays the captured graph -- and once at 1e-10."""
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
          "beam128L4_brick": lambda: scenes.fat_beam(128, 4, device=dev)}[scene]()   # (AVS_BRICK in the environment)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    pi = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pi.levels)
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
    out, xs = {}, []
    for k, t in enumerate((tol, tol, 1e-10), 1):
        info = s.dist_solve(t, 5000)
        fmt = s.matrix_format()
        out.update({f"iterations{k}": info.iterations, f"converged{k}": info.converged, f"error{k}": info.error,
                    f"reliable_updates{k}": fmt.reliable_updates})
        xs.append(s.dist_solution())                     # hosted group: owned entries, zeros elsewhere
        if k == 1:
            out.update(float_vectors=fmt.float_vectors, reliable_updates=fmt.reliable_updates, resident=info.resident,
                       brick_tiles=fmt.brick_tiles)
    ci = s.dist_comm_info()
    out.update(n_halo=s.plan_sizes.n_halo, direct=1 if ci["transport"] == "direct" else 0, rccl_calls=ci["rccl_calls_per_iteration"],
               selftest_rounds=ci["selftest_rounds"], selftest_bad=ci["selftest_bad_entries"])
    np.save(os.path.join(workdir, f"x_{rank}.npy"), np.stack(xs))
    np.save(os.path.join(workdir, f"names_{rank}.npy"), np.array(list(out)))
    np.save(os.path.join(workdir, f"info_{rank}.npy"), np.array([float(v) for v in out.values()]))
    # keep the comm block alive until every rank has finished (a peer may still be reading its own copy of the flags)
    open(os.path.join(workdir, f"done_{rank}"), "w").write("ok")
    for q in range(world):
        wait_for(os.path.join(workdir, f"done_{q}"))
    s.close()


if __name__ == "__main__":
    main()
