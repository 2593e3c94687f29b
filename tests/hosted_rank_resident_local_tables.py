"""One rank of a HOSTED multi-process solve of a variable-viscosity system in the CU-resident loop with local value tables
(tests/test_gpu_resident_local_tables.py::test_local_tables_across_ranks).

As tests/hosted_rank_resident_f32.py (blob hand-over through files, both processes on cuda:0), an fp64 context, with
AVS_RESIDENT_LOCAL_TABLES=1 and AVS_CG_RESIDENT_CUS in the environment: every rank plans its local [owned | halo] system with local
tables and runs k_cg_resident<.., double, true> on its share of the CUs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hosted_rank import wait_for  # noqa: E402


def make_context(scene, dev):
    """The context of `scene` with its system assembled by nobody yet (fields set, pyramid fed)."""
    from adaptiveviscositysolver_amd import ViscositySolve, scenes
    from util import build_pyramid, feed
    sc = {"beam64_varvisc": lambda: scenes.fat_beam(64, 3, variable_viscosity=True),
          "beam128_varvisc": lambda: scenes.fat_beam(128, 3, variable_viscosity=True)}[scene]()
    dsc = scenes.to_device(sc, dev)
    pyr = build_pyramid(dsc)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pyr.levels, device=0, field_res=sc.field_res)
    feed(s, pyr)
    s.set_scene_fields(scenes.crop_to_field(dsc))
    return s


def main():
    import ctypes as C

    import torch
    from adaptiveviscositysolver_amd import capi
    workdir, rank, world, scene, tol = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], float(sys.argv[5])
    s = make_context(scene, torch.device("cuda:0"))
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
    capi.check(s.lib.avs_dist_import_blobs(s.h, buf))
    runs, xs = [], []
    for _ in range(2):                                   # twice: the second solve re-uses the plan
        info = s.dist_solve(tol, 5000)
        runs.append((info.iterations, info.converged, info.resident, info.error))
        xs.append(s.dist_solution())                     # hosted group: owned entries, zeros elsewhere
    np.save(os.path.join(workdir, f"x_{rank}.npy"), xs[0])
    np.save(os.path.join(workdir, f"info_{rank}.npy"), np.array([*runs[0], *runs[1]], np.float64))
    # keep the comm block alive until every rank has finished (a peer may still be reading its own copy of the flags)
    open(os.path.join(workdir, f"done_{rank}"), "w").write("ok")
    for q in range(world):
        wait_for(os.path.join(workdir, f"done_{q}"))
    s.close()


if __name__ == "__main__":
    main()
