"""A plain `bench.py` run (no --full) times the steps and prints the headline line only; `--dump-outputs DIR` writes what the last timed
step computed: the solution of the same system a caller of the library gets from one solve."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT, rel_l2

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_steps_solution(tmp_path, built_lib):
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "64", "--levels", "3", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(d)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    head = json.loads(lines[0])
    assert head["metric"] == "cg_iterations_per_sec" and head["value"] > 0 and head["ms_per_step"] > 0 and head["steps"] == 2
    for k in ("cpu_baseline", "extra", "full_record"):   # --full only
        assert k not in head
    x = np.load(d / "solution.npy")
    it, conv, err, _ = np.load(d / "solve_info.npy").tolist()
    assert x.dtype == np.float64 and x.size == head["config"]["n_dofs"] and np.all(np.isfinite(x))
    assert conv == 1 and it == head["config"]["cg_iterations_per_step"] and 0 < err <= 1e-3

    import torch
    from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, scenes
    sc = scenes.fat_beam(64, 3, device=torch.device("cuda:0"))
    pp = DevicePrepass(sc.res, sc.dx, sc.levels, device=0)
    pinfo = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pinfo.levels, device=0)
    pp.apply(s)
    s.set_scene_fields(sc)
    pp.close()
    s.assemble()
    info = s.solve(1e-3, 2500)
    assert info.iterations == it
    assert rel_l2(x, s.solution()) < 1e-10
    s.close()
