"""avs_sample_velocity on the 512^3 fat beam: points per second for 10^6 .. 10^7 uniformly random points inside the liquid's bounding box,
in random order and in Morton order (the same points sorted by the interleaved bits of their level-0 cell), device arrays.
For context: the transfer's interpolated faces per second on the same scene (regular DOF faces with an UNASSIGNED octree index over the
time of one transfer that reuses the node grids, i.e. scatter + apply + unscatter -- what a sample call runs around its kernel).
`python tools/point_sample_probe.py [n ...]` prints one JSON line per measurement."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adaptiveviscositysolver_amd import DevicePrepass, ViscositySolve, capi, scenes  # noqa: E402


def part1by2(v):
    v = v & 0x3ff
    v = (v | (v << 16)) & 0x30000ff
    v = (v | (v << 8)) & 0x300f00f
    v = (v | (v << 4)) & 0x30c30c3
    v = (v | (v << 2)) & 0x9249249
    return v


def timed(fn, repeats=5):
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    counts = [int(float(a)) for a in sys.argv[1:]] or [1_000_000, 3_000_000, 10_000_000]
    dev = torch.device("cuda:0")
    sc = scenes.fat_beam(512, 4, device=dev)
    pp = DevicePrepass(sc.res, sc.dx, sc.levels)
    pi = pp.run(sc.liquid, sc.solid)
    s = ViscositySolve(sc.res, sc.dx, sc.dt, pi.levels)
    pp.apply(s)
    s.set_scene_fields(sc)
    s.assemble()
    s.solve(1e-3, 2500)
    # the transfer, for context
    outs = [torch.empty_like(v) for v in sc.velocity]
    tr = lambda: capi.check(s.lib.avs_transfer_to_regular_grid(s.h, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), capi.MEM_DEVICE))
    tr()
    t_tr = timed(tr)
    faces = sum(int(((torch.from_numpy(pp.regular_index(a)) >= 0) & (torch.from_numpy(pp.index(capi.INDEX_VELOCITY, 0, a)) == capi.UNASSIGNED)).sum())
                for a in range(3))
    print(json.dumps({"what": "transfer", "ms": round(t_tr * 1e3, 3), "interpolated_faces": faces, "faces_per_s": round(faces / t_tr)}), flush=True)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    half = torch.tensor([0.45, 0.225, 0.225], device=dev)
    for n in counts:
        p = (0.5 + (torch.rand((n, 3), generator=g, device=dev) * 2 - 1) * half).to(torch.float32).contiguous()
        c = torch.floor(p / sc.dx).to(torch.int64)
        key = part1by2(c[:, 0]) | (part1by2(c[:, 1]) << 1) | (part1by2(c[:, 2]) << 2)
        pm = p[torch.argsort(key)].contiguous()
        for order, pts in (("random", p), ("morton", pm)):
            v, inside = s.sample_velocity(pts)
            t = timed(lambda: s.sample_velocity(pts))
            print(json.dumps({"what": "sample", "order": order, "points": n, "ms": round(t * 1e3, 3), "points_per_s": round(n / t),
                              "inside_fraction": round(float(inside.float().mean()), 4)}), flush=True)
        del p, pm, c, key


if __name__ == "__main__":
    main()
