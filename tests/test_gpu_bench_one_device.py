"""Rehearsal of `bench.py --gpus N` on ONE GPU (round-3 review, item 2): the branch an 8-GPU node will execute -- launcher, process
group, distributed assembly, transport connection + self-test, paranoid verification against the single-GPU solve, timed solves,
max-over-ranks timing, per-rank gather and the JSON `dist` block -- with every rank on cuda:0 (`--one-device`: gloo for the script's
own collectives, hosted group + HIP IPC for the library).  What it cannot exercise: RCCL with more than one rank, xGMI."""
import json
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ranks,vtol", [(2, 1e-8), (8, 1e-4)])
def test_bench_gpus_n_on_one_device(ranks, vtol, built_lib):
    """(ranks that share one GPU are time-sliced: every flag wait costs a context switch, ~20 ms per iteration at 2 ranks and ~140 ms at
    8 -- the 8-rank case verifies at 1e-4 to stay within minutes; both passed at 1e-8 and 128^3 once: profiles/r04_notes.md)"""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--one-device", "--n", "64", "--levels", "3",
           "--steps", "1", "--warmup", "1", "--verify-tol", str(vtol), "--no-cpu-baseline", "--no-extra", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    head = json.loads(lines[0])
    assert head["n_gpus"] == ranks and head["value"] > 0 and head["scaling"] == "strong" and head["dist"]["verified"]
    out = json.load(open(os.path.join(ROOT, head["full_record"])))   # (the stdout line is the <= 4 KB headline; the whole record is a file)
    assert out["n_gpus"] == ranks and out["value"] == pytest.approx(head["value"], rel=1e-4)
    d = out["dist"]
    assert len(d["per_rank"]) == ranks and sum(r["n_own"] for r in d["per_rank"]) == out["config"]["n_dofs"]
    assert d["transport"] == "direct" and d["selftest_rounds"] > 0 and d["selftest_bad_entries"] == 0
    v = d["verification"][-1]
    assert v["ok"] and v["paranoid"] and len(v["solves"]) == 3
    assert all(s["converged"] and s["rel_l2_vs_single_gpu"] < max(1e-6, 100 * vtol) for s in v["solves"])


def test_bench_slab_local_frame_on_one_device(built_lib):
    """`bench.py --gpus 2 --one-device --slab-local`: after the timed solves one more frame runs through the slab-local path -- the pre-pass of
    every rank's window with this script's own all-reduce (torch.distributed on gloo through avs_prepass_set_slab's callback), the window lent
    to the context, avs_dist_assemble on it -- and its solve reproduces the solve on the replicated-index assembly."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--one-device", "--slab-local", "--n", "64", "--levels", "3",
           "--steps", "1", "--warmup", "1", "--verify-tol", "1e-8", "--no-cpu-baseline", "--no-extra", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    head = json.loads(lines[-1])
    assert head["dist"]["slab_local_ok"]
    out = json.load(open(os.path.join(ROOT, head["full_record"])))
    sl = out["dist"]["slab_local"]
    assert sl["ok"] and sl["rel_l2_vs_replicated"] < 1e-6 and abs(sl["iterations"] - sl["iterations_replicated_cuts"]) <= 3
    assert len(sl["prepass_ms_per_rank"]) == 2 and len(sl["cuts"]) == 3 and sl["cuts"][0] == 0 and sl["cuts"][-1] == 64
    assert all(0 < f <= 1 for f in sl["window_fraction_of_dofs_per_rank"])
