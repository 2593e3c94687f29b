"""The device builder of the brick-structured SpMV form and its kernel k_spmv_brick on the planted cases of tests/brick_edges.py, through
avs_brick_form_probe (include/avs_probe.h): build_brick_form on the case's CSR, then the kernel the loops launch.

  builder   the header words the device wrote equal the model's (tests/brick_model.py) word for word, the counts equal the model's sums
  product   y is bit-exact against a plain left-to-right row sum without FMA -- fp64: the C oracle's spmv_csr; float: util.float_row_sums;
            mixed: within one float ulp of the rounded fp64 row sum of the narrowed x (the bound of test_gpu_mixed_precision.py) -- for
            the plain and the fused launch of each kernel, for the grids 1, 3, 8, 16, the number of tiles and the default, under the walks
            0 (eighths), 1 (dealt chunks) and 2 (planned), and is the same vector for all of them.  The library clamps the grid to the
            number of tiles; the reported grid is asserted.
  fused dot the same value twice; against math.fsum of the terms within (2T + 1) u S + (G + 16) 2^-53 S with u = 2^-53 (fp64, mixed), and
            (2T + 2) 2^-24 S + (G + 16) 2^-53 S (float): G the grid, T the most tiles a workgroup walks, S = sum |x_i y_i|.  The terms are
            x_i (narrowed for the float kernels) times the row sum the kernel multiplies with: its y for the fp64 and the float kernel, and
            for the mixed kernel the fp64 row sum BEFORE it is rounded to the float y -- the kernel's dot uses the unrounded sum, and
            rounding y alone moves every term by up to 2^-24 |x_i y_i|, 2^29 times the unit of that bound.
            The partials fold, in order, to exactly the dot the entry returns.  BrickForm::plan_walk lays nothing out when a workgroup would
            stay without tiles (info.planned == 0: the strided walk runs instead) and the strided walks of a grid clamped to the tiles
            leave no workgroup idle either, so no partial of these launches is the 0.0 of an idle workgroup.
  done      with the flag set, y (poisoned with NaN) and the partials come back untouched.
"""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

import brick_edges as E
import brick_model as M
import util
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GRIDS = (1, 3, 8, 16, "ntiles", 0)
WALKS = (0, 1, 2)
KERNELS = (("fp64", 0), ("float", 2), ("mixed", 4))       # name, flag (capi.BRICK_PROBE_F32 / _MIXED)
FORCED_VC = ("mix_walk", "many_tiles", "sw_park+1", "shapes", "halo", "coarse_neighbour", "rows_full_brick", "runs_fast+1")
WIDE = ("sw_1025", "emode_cap+1", "mix_walk", "halo", "extras_xslots+1")


@pytest.fixture(autouse=True)
def _force_the_form(monkeypatch):
    """AVS_BRICK=1 takes the value-code variant regardless of its share of pattern rows; the share asked of the dictionary variant is an
    option of its own (AVS_BRICK_MIN_REGULAR): 0, so that cases whose rows are mostly streamed still get their form"""
    monkeypatch.setenv("AVS_BRICK", "1")
    monkeypatch.setenv("AVS_BRICK_MIN_REGULAR", "0")
    for k in ("AVS_BRICK_DEBUG", "AVS_BRICK_GRID", "AVS_VALUE_PACK", "AVS_COLUMN_WINDOWS", "AVS_VALUE_INDEX", "AVS_TILE_TABLES", "AVS_BRICK_VALUE_CODES"):
        monkeypatch.delenv(k, raising=False)


class Device:
    """one case on the device at a time"""

    def __init__(self, c):
        import torch
        from adaptiveviscositysolver_amd import capi
        self.capi, self.lib, self.c, self.torch = capi, capi.load_probe(), c, torch
        dev = torch.device("cuda:0")
        self.rp = torch.from_numpy(c.row_ptr).to(dev)
        self.col = torch.from_numpy(c.col).to(dev)
        self.val = torch.from_numpy(c.val).to(dev)
        self.dof = torch.from_numpy(c.dof).to(dev)
        self.x = torch.from_numpy(c.x).to(dev)
        self.y = torch.empty(c.n_rows, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

    def run(self, flags=0, grid=0, walk=1, headers=False, partials=None, poison=True):
        c, capi = self.c, self.capi
        info = capi.BrickFormInfo()
        dot = C.c_double(0.0)
        cap = 4 * (len(c.model().tiles) + 1)
        hdr = np.full((cap, 16), -1, np.int32) if headers else None
        if poison:
            self.y.fill_(float("nan"))
        self.torch.cuda.synchronize()
        status = self.lib.avs_brick_form_probe(c.n_rows, c.n_cols, self.rp.data_ptr(), self.col.data_ptr(), self.val.data_ptr(), self.dof.data_ptr(),
                                                 c.nx, c.ny, c.nz, c.levels, self.x.data_ptr(), self.y.data_ptr(), flags, grid, walk, C.byref(dot),
                                                 None if partials is None else partials.ctypes.data, 0 if partials is None else len(partials),
                                                 C.byref(info), None if hdr is None else hdr.ctypes.data, cap, None)
        if status == capi.EHIP:     # a device error: nothing more is launched in this session
            pytest.exit(f"{c.name}: HIP error in avs_brick_form_probe (flags {flags}, grid {grid}, walk {walk}): "
                        f"{self.lib.avs_last_error().decode('utf-8', 'replace')}", returncode=3)
        capi.check(status)
        return info, self.y.cpu().numpy(), dot.value, hdr


_REF = {}


def reference(c):
    """the plain row sums of a case, computed once and shared (not to be written to)"""
    if c.name not in _REF:
        xf = c.x.astype(np.float32).astype(np.float64)
        rp64 = c.row_ptr.astype(np.int64)
        _REF[c.name] = dict(fp64=orc.spmv_csr(rp64, c.col, c.val, c.x), float=util.float_row_sums(c.row_ptr, c.col, c.val, c.x).astype(np.float64),
                            mixed64=orc.spmv_csr(rp64, c.col, c.val, xf), xf=xf)
    return _REF[c.name]


def check_headers(c, m, info, hdr, what):
    assert info.ready == 1, (c.name, what, "form not ready")
    assert info.tiles == len(m.tiles), (c.name, what, "tiles", info.tiles, len(m.tiles))
    assert (info.pattern_rows, info.streamed_rows, info.streamed_words, info.halo_tiles, info.patterns) == \
        (m.pattern_rows, m.streamed_rows, m.streamed_words, m.halo_tiles, m.patterns), (c.name, E.edge_of(c.name), what, "counts of the form against the model's sums")
    names = ("row0", "nrows", "npat", "nruns", "npq", "nprow", "srow0", "nsrows", "sword0", "nsw", "rd0", "halo", "code0", "table0", "ntv", "w15")
    for pos, t in enumerate(m.order):
        for w in M.HEADER_WORDS_COMPARED:
            assert hdr[pos, w] == m.headers[t, w], \
                f"{c.name} <{E.edge_of(c.name)}> ({what}): tile {t} ({m.tiles[t].kind}, rows {m.tiles[t].row0}+{m.tiles[t].nrows}) at place {pos} of the tile list: header " \
                f"word {w} ({names[w]}) is {hdr[pos, w]}, the model says {m.headers[t, w]}"


def check_product(c, kname, y, what):
    ref = reference(c)
    if kname == "mixed":
        want = ref["mixed64"].astype(np.float32)
        ulps = np.abs(y - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        assert np.array_equal(y, y.astype(np.float32).astype(np.float64)) and float(ulps.max()) <= 1.0, \
            f"{c.name} <{E.edge_of(c.name)}> ({what}): row {int(ulps.argmax())} is {float(ulps.max()):.2f} float ulp from the rounded fp64 row sum"
        return
    want = ref[kname]
    bad = np.flatnonzero(y.view(np.int64) != want.view(np.int64))
    if len(bad):
        tiles = c.model().tiles
        t = max(i for i, T in enumerate(tiles) if T.row0 <= bad[0])
        raise AssertionError(f"{c.name} <{E.edge_of(c.name)}> ({what}): {len(bad)} rows differ from the plain row sum, first row {bad[0]} (tile {t}, {tiles[t].kind}, rows "
                             f"{tiles[t].row0}+{tiles[t].nrows}): {y[bad[0]]!r} against {want[bad[0]]!r}")


def check_dot(c, kname, info, y, dot, what):
    ref = reference(c)
    x = c.x[:c.n_rows] if kname == "fp64" else ref["xf"][:c.n_rows]
    rows = ref["mixed64"] if kname == "mixed" else y     # (mixed: the unrounded fp64 row sums, see the module's docstring)
    terms = x * rows
    S, G, T = float(np.abs(terms).sum()), info.grid, info.max_walk
    bound = ((2 * T + 2) * 2.0 ** -24 if kname == "float" else (2 * T + 1) * 2.0 ** -53) * S + (G + 16) * 2.0 ** -53 * S
    err = abs(dot - math.fsum(terms.tolist()))
    assert err <= bound, f"{c.name} <{E.edge_of(c.name)}> ({what}): fused dot off by {err:.3e}, bound {bound:.3e} (G {G}, T {T}, S {S:.3e})"
    return err / bound if bound else 0.0


def sweep(c, d, m, vc_flag, what, kernels=KERNELS, grids=GRIDS, walks=WALKS):
    """every kernel, plain and fused, every grid and walk: product, one y for all, grid, dot; returns the lines of the report"""
    capi = d.capi
    ntiles, ran, worst = len(m.tiles), [], 0.0
    for kname, kflag in kernels:
        first = None
        for g in grids:
            grid = ntiles if g == "ntiles" else g
            for walk in walks:
                for fused in (0, 1):
                    tag = f"{what} {kname} {'fused' if fused else 'plain'} grid {g} walk {walk}"
                    info, y, dot, _ = d.run(flags=kflag | vc_flag | (capi.BRICK_PROBE_FUSED_DOT if fused else 0), grid=grid, walk=walk)
                    assert info.ready == 1 and info.vc == (1 if (c.vc or vc_flag) else 0), (c.name, tag, info.ready, info.vc)
                    if grid:
                        assert info.grid == min(grid, ntiles), (c.name, tag, "the library clamps the grid to the tiles", info.grid)
                    else:
                        assert 1 <= info.grid <= ntiles, (c.name, tag, info.grid)
                    assert info.planned == 0 or (walk == 2 and info.grid % 8 == 0), (c.name, tag)
                    check_product(c, kname, y, tag)
                    if first is None:
                        first = y
                    assert np.array_equal(first.view(np.int64), y.view(np.int64)), f"{c.name} <{E.edge_of(c.name)}> ({tag}): y differs from the first launch of this kernel"
                    if fused:
                        worst = max(worst, check_dot(c, kname, info, y, dot, tag))
                        if (g, walk) in ((1, 1), (8, 2), (0, 0)):     # the same grid and walk twice: the same dot, and the partials fold to it
                            part = np.full(info.grid + 3, 7.25)
                            info2, y2, dot2, _ = d.run(flags=kflag | vc_flag | capi.BRICK_PROBE_FUSED_DOT, grid=grid, walk=walk, partials=part)
                            assert dot2 == dot and info2.grid == info.grid, f"{c.name} <{E.edge_of(c.name)}> ({tag}): fused dot {dot2!r} after {dot!r}"
                            s = 0.0
                            for v in part[:info.grid]:
                                s += float(v)
                            assert s == dot and np.all(part[info.grid:] == 7.25), (c.name, tag, "partials")
                    ran.append((kname, fused, g, walk, info.grid, info.max_walk, info.planned))
    grids_ran = sorted({(r[2], r[4]) for r in ran}, key=str)
    return (f"{c.name} <{E.edge_of(c.name)}> ({what}): tiles {''.join('e' if T.kind == 'E' else ('x' if T.kind == 'GE' else ('S' if T.nsw else 'G')) for T in m.tiles)} "
            f"(G pattern tile, S with streamed rows, e E tile, x redone as E) | kernels {[k for k, _ in kernels]} x plain, fused | "
            f"grids asked -> used {grids_ran} | walks {list(walks)}, planned {sum(r[6] for r in ran)} launches | most tiles per workgroup "
            f"{max(r[5] for r in ran)} | {len(ran)} launches, worst dot error {worst:.2f} of its bound")


@pytest.mark.parametrize("name", E.NAMES)
def test_case(name, capsys):
    c = E.cases()[name]
    m = c.model()
    d = Device(c)
    vc_flag = d.capi.BRICK_PROBE_VALUE_CODES if c.force_vc else 0
    t0 = time.time()
    info, y, _, hdr = d.run(flags=vc_flag, headers=True)
    assert info.vc == (1 if c.vc else 0), (name, "value-code variant", info.vc)
    if c.racy_extras:
        assert info.ready == 1 and info.tiles == len(m.tiles)      # (which candidates get a slot is racy: the product below is not)
    else:
        check_headers(c, m, info, hdr, "builder")
    line = sweep(c, d, m, vc_flag, "as planted")
    # done: y and the partials stay as they were
    part = np.full(info.tiles + 2, 7.25)
    for kname, kflag in KERNELS:
        i2, y2, dot2, _ = d.run(flags=kflag | vc_flag | d.capi.BRICK_PROBE_FUSED_DOT | d.capi.BRICK_PROBE_DONE, partials=part)
        assert i2.ready == 1 and np.all(np.isnan(y2)) and np.all(part == 7.25) and dot2 == 0.0, (name, kname, "done flag")
    with capsys.disabled():
        print(f"\n{line} | {time.time() - t0:.1f} s")


@pytest.mark.parametrize("name", FORCED_VC)
def test_forced_value_codes(name, capsys):
    """a dictionary case again with the value-code variant forced: geometry-only patterns, a value table per tile"""
    c = E.cases()[name]
    assert not c.vc
    m = c.model(vc=True)
    d = Device(c)
    flag = d.capi.BRICK_PROBE_VALUE_CODES
    info, y, _, hdr = d.run(flags=flag, headers=True)
    assert info.vc == 1 and info.wide == 1
    check_headers(c, m, info, hdr, "value codes forced")
    line = sweep(c, d, m, flag, "value codes forced", grids=(1, 3, 8, 0))
    with capsys.disabled():
        print("\n" + line)


@pytest.mark.parametrize("env", ({"AVS_VALUE_PACK": "0"}, {"AVS_VALUE_PACK": "0", "AVS_COLUMN_WINDOWS": "0"}), ids=("unpacked", "unpacked_no_windows"))
@pytest.mark.parametrize("name", WIDE)
def test_wide_streamed_words(name, env, monkeypatch, capsys):
    """64-bit streamed words (column | code << 32): the same tiles, the same product"""
    c = E.cases()[name]
    d = Device(c)
    info, y, _, hdr = d.run(headers=True)
    assert info.ready == 1 and info.wide == 0 and info.col_bits > 0, (name, "the default form packs code and column into 32 bits", info.wide, info.col_bits)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    info, y, _, hdr = d.run(headers=True)
    assert info.wide == 1 and info.vc == 0, (name, env, info.wide, info.col_bits)
    check_headers(c, c.model(), info, hdr, f"wide {env}")
    line = sweep(c, d, c.model(), 0, f"wide {sorted(env)}", grids=(1, 3, 0), walks=(0, 1))
    with capsys.disabled():
        print("\n" + line)


def test_refusals():
    """an empty row and rows out of brick order are refused on the host, before anything is launched"""
    from adaptiveviscositysolver_amd import capi
    c = E.cases()["rows_min"]
    d = Device(c)
    rp = c.row_ptr.copy()
    rp[5] = rp[4]                       # row 4 is empty (row 5 takes its entries)
    d.rp = d.torch.from_numpy(rp).to(d.x.device)
    with pytest.raises(capi.AvsError) as e:
        d.run()
    assert e.value.status == capi.EINVAL and "empty" in str(e.value)
    d = Device(c)
    dof = c.dof.copy()
    dof[[0, c.n_rows - 1]] = dof[[c.n_rows - 1, 0]]
    d.dof = d.torch.from_numpy(dof).to(d.x.device)
    with pytest.raises(capi.AvsError) as e:
        d.run()
    assert e.value.status == capi.EINVAL and "brick-major" in str(e.value)
    assert np.all(np.isnan(d.y.cpu().numpy()))          # nothing was launched on y
