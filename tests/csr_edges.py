"""Named CSR matrices at the edges of the lossless SpMV storage forms, and the rule that picks the form.

`build_matrix_index` (csrc/avs_reorder.hip) gives a matrix one of five storage forms:

  * one dictionary of <= 2048 values, staged in LDS: packed 4-B words (code << column bits | column) when bits(n) + bits(table) <= 32,
    otherwise windowed 4-B words (the columns of a 512-row tile lie in <= 64 aligned windows of 2^14 ids), otherwise 6 B (code + column);
  * one dictionary per 512-row tile when no tile holds more than 3072 distinct values and the tables (8 B per entry) stay within a
    quarter of the 8-B value stream: windowed 4-B words, or 6 B;
  * one dictionary of <= 65536 values read through L1: packed when the bits allow, else 6 B;
  * plain 12-B CSR.

`expected_format` restates that choice in numpy, for the default environment and for the AVS_* switches in ENVS.  `cases()` builds the
matrices (host numpy, seeded); every case names the edge it sits on and carries the facts that make it so (`Case.props`), which
tests/test_csr_edges.py checks without going through the rule.  Values are drawn from palettes in [0.25, 1) so that `spd_version` can
turn a case into a symmetric, strictly diagonally dominant system with the same value palette.
"""
from __future__ import annotations

import numpy as np

TILE_ROWS = 512          # rows per SpMV tile (spmv_tile_rows) and per tile-local dictionary
PASS = 4096              # products per pass of the value-indexed kernel (kTileCap)
WIN_BITS = 14            # column windows: aligned runs of 2^14 ids ...
WIN_SLOTS = 64           # ... at most 64 per tile
LDS_TABLE = 2048         # one dictionary staged in LDS
TLT_LDS = 1024           # tile-local entries staged in LDS (a tile with more takes the kernel's `big` path)
TILE_MAX_KEYS = 3072     # distinct values a tile-local dictionary may hold
DICT_MAX = 65536         # one dictionary read through L1
EMPTY_BITS = 0xFFFF_FFFF_FFFF_FFFF   # the hash tables' empty-slot key: a matrix holding it gets no dictionary

ENVS = {
    "default": {},
    "no_pack": {"AVS_VALUE_PACK": "0"},
    "no_windows": {"AVS_COLUMN_WINDOWS": "0"},
    "no_tiles": {"AVS_TILE_TABLES": "0"},
    "no_index": {"AVS_VALUE_INDEX": "0"},
}
FMT_FIELDS = ("value_table_size", "column_bits", "bytes_per_nonzero", "tile_local_tables", "column_windows")


def bits_for(count):
    """bits that hold 0 .. count-1 (at least 1), as in csrc/avs_reorder.hip"""
    b = 1
    while (1 << b) < count:
        b += 1
    return b


def _tile_of_entry(row_ptr):
    rp = np.asarray(row_ptr, dtype=np.int64)
    n = len(rp) - 1
    return np.repeat(np.arange(n, dtype=np.int64) // TILE_ROWS, np.diff(rp))


def _per_tile_unique(tiles, keys, ntiles):
    """number of distinct keys in every tile"""
    if len(keys) == 0:
        return np.zeros(ntiles, dtype=np.int64)
    order = np.lexsort((keys, tiles))
    t, k = tiles[order], keys[order]
    new = np.ones(len(k), dtype=bool)
    new[1:] = (t[1:] != t[:-1]) | (k[1:] != k[:-1])
    return np.bincount(t[new], minlength=ntiles)


def expected_format(row_ptr, col, val, env=None):
    """The avs_matrix_format fields (FMT_FIELDS) build_matrix_index gives this CSR, n columns, under `env` (AVS_* -> "0"/"1")."""
    env = env or {}
    on = lambda k: env.get(k, "1") != "0"
    rp = np.asarray(row_ptr, dtype=np.int64)
    n = len(rp) - 1
    nnz = int(rp[-1])
    bits = np.ascontiguousarray(val, dtype=np.float64).view(np.uint64)
    col = np.asarray(col, dtype=np.int64)
    plain = dict(value_table_size=0, column_bits=0, bytes_per_nonzero=12, tile_local_tables=0, column_windows=0)
    if nnz == 0 or not on("AVS_VALUE_INDEX"):
        return plain
    sentinel = bool((bits == np.uint64(EMPTY_BITS)).any())
    distinct = len(np.unique(bits))
    global_size = 0 if sentinel or distinct > DICT_MAX else distinct
    ntiles = (n + TILE_ROWS - 1) // TILE_ROWS
    tiles = _tile_of_entry(rp)

    def windows_fit():
        return int(_per_tile_unique(tiles, col >> WIN_BITS, ntiles).max()) <= WIN_SLOTS

    def packs(size):
        return on("AVS_VALUE_PACK") and bits_for(n) + bits_for(size) <= 32

    if 0 < global_size <= LDS_TABLE:
        if packs(global_size):
            return dict(plain, value_table_size=global_size, column_bits=bits_for(n), bytes_per_nonzero=4)
        win = on("AVS_COLUMN_WINDOWS") and windows_fit()
        return dict(plain, value_table_size=global_size, bytes_per_nonzero=4 if win else 6, column_windows=int(win))
    if on("AVS_TILE_TABLES"):
        per_tile = _per_tile_unique(tiles, bits, ntiles)
        total = int(per_tile.sum())
        if not sentinel and per_tile.max() <= TILE_MAX_KEYS and 0 < total and total * 8 <= nnz * 2:
            win = on("AVS_COLUMN_WINDOWS") and windows_fit()
            return dict(plain, value_table_size=total, bytes_per_nonzero=4 if win else 6, tile_local_tables=1, column_windows=int(win))
    if global_size > 0:
        if packs(global_size):
            return dict(plain, value_table_size=global_size, column_bits=bits_for(n), bytes_per_nonzero=4)
        return dict(plain, value_table_size=global_size, bytes_per_nonzero=6)
    return plain


def instantiation(fmt, row_ptr=None, val=None):
    """Which k_spmv_vi2 / plain kernel a form reaches: a short name (+ "big" when a tile-local dictionary exceeds TLT_LDS)."""
    if fmt["value_table_size"] == 0:
        return "plain CSR"
    if fmt["tile_local_tables"]:
        name = "tile dictionary " + ("windowed" if fmt["column_windows"] else "6 B")
        if row_ptr is not None:
            rp = np.asarray(row_ptr, dtype=np.int64)
            ntiles = (len(rp) - 1 + TILE_ROWS - 1) // TILE_ROWS
            per_tile = _per_tile_unique(_tile_of_entry(rp), np.ascontiguousarray(val).view(np.uint64), ntiles)
            if per_tile.max() > TLT_LDS:
                name += " + big"
        return name
    where = "LDS dictionary" if fmt["value_table_size"] <= LDS_TABLE else "L1 dictionary"
    if fmt["column_bits"] > 0:
        return where + " packed"
    return where + (" windowed" if fmt["column_windows"] else " 6 B")


class Case:
    def __init__(self, name, row_ptr, col, val, props, f32=False, spd=True):
        self.name = name
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.n = len(self.row_ptr) - 1
        self.props = props      # the facts the name claims (checked by tests/test_csr_edges.py)
        self.f32 = f32          # small enough for the float row-sum reference
        self.spd = spd          # has a solvable symmetric version (spd_version)

    def __repr__(self):
        return f"Case({self.name}, n={self.n}, nnz={int(self.row_ptr[-1])})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------------------
def _csr(n, rows, cols, vals):
    """CSR from entries; the order of the entries inside a row is kept"""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp, np.asarray(cols, dtype=np.int64)[order], np.asarray(vals, dtype=np.float64)[order]


def _palette(k, rng, lo=0.25, hi=1.0):
    """k distinct doubles in [lo, hi), increasing, with random low bits"""
    return lo + (hi - lo) * (np.arange(k) + rng.uniform(0.05, 0.95, k)) / k


def _cover(count, palette, rng):
    """`count` draws from `palette` that use every entry at least once"""
    k = len(palette)
    assert count >= k, (count, k)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, count - k)])
    return palette[rng.permutation(idx)]


def _band(n, per_row, rng, width=3):
    """diagonal + (per_row - 1) columns within +-width of it, wrapped into [0, n) (every row has exactly per_row entries)"""
    rows = np.repeat(np.arange(n, dtype=np.int64), per_row)
    off = rng.integers(-width, width + 1, (n, per_row))
    off[:, 0] = 0
    cols = (np.arange(n, dtype=np.int64)[:, None] + off) % max(n, 1)
    return rows, cols.ravel()


def _tile_values(n, rows, palettes, rng):
    """values of the entries of every tile drawn from that tile's palette (each palette entry used once at least)"""
    vals = np.empty(len(rows), dtype=np.float64)
    tiles = rows // TILE_ROWS
    for t, pal in enumerate(palettes):
        m = np.nonzero(tiles == t)[0]
        vals[m] = _cover(len(m), pal, rng)
    return vals


def _disjoint_palettes(sizes, rng):
    """one palette per tile, the tiles' value ranges disjoint"""
    k = len(sizes)
    return [_palette(s, rng, 0.25 + 0.75 * t / k, 0.25 + 0.75 * (t + 1) / k) for t, s in enumerate(sizes)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def _distinct_cases():
    out = []
    rng = np.random.default_rng(101)
    rows, cols = _band(3000, 5, rng)
    out.append(Case("dist_1", *_csr(3000, rows, cols, np.full(len(rows), 0.5)), {"distinct": 1}, f32=True))

    rng = np.random.default_rng(102)
    rows, cols = _band(6000, 5, rng)
    out.append(Case("dist_2048", *_csr(6000, rows, cols, _cover(len(rows), _palette(2048, rng), rng)), {"distinct": 2048}))

    # 2049 values, 128 per tile: tile t draws from the palette slice [86 t, 86 t + 128) (mod 2049) -- together they cover all of it
    rng = np.random.default_rng(103)
    n = 24 * TILE_ROWS
    rows, cols = _band(n, 8, rng)
    pal = _palette(2049, rng)
    pals = [pal[(86 * t + np.arange(128)) % 2049] for t in range(24)]
    out.append(Case("dist_2049", *_csr(n, rows, cols, _tile_values(n, rows, pals, rng)),
                    {"distinct": 2049, "max_tile_distinct": 128}, f32=True))

    # one dictionary of 65536 / 65537 values; two entries per row, each value in ~2 of them: the tile tables would be about a whole
    # value stream (not within a quarter of it)
    for name, n, k in (("dist_65536_n65536", 65536, 65536), ("dist_65536_n65537", 65537, 65536), ("dist_65537", 65537, 65537)):
        rng = np.random.default_rng(104 + n + k)
        rows, cols = _band(n, 2, rng, width=40)
        r, c, v = _csr(n, rows, cols, _cover(len(rows), _palette(k, rng), rng))
        out.append(Case(name, r, c, v, {"n": n, "distinct": k, "tile_total_over_quarter": True}))
    return out


def _tile_cases():
    out = []
    n = 16 * TILE_ROWS
    for k in (1024, 1025, 3072, 3073):   # tile 0: k distinct values; tiles 1..15: 128 each (global > 2048, the tables a small share)
        rng = np.random.default_rng(200 + k)
        rows, cols = _band(n, 8, rng)
        pals = _disjoint_palettes([k] + [128] * 15, rng)
        out.append(Case(f"tile_{k}", *_csr(n, rows, cols, _tile_values(n, rows, pals, rng)),
                        {"tile_distinct": {0: k, 1: 128}, "distinct": k + 15 * 128}, f32=(k == 1025)))
    # the quarter-of-the-stream limit: 8 tiles x 4 entries per row = 16384 non-zeros; tables of 4096 (= nnz / 4) and 4097 entries
    n = 8 * TILE_ROWS
    for name, k0 in (("quarter_in", 512), ("quarter_out", 513)):
        rng = np.random.default_rng(210 + k0)
        rows, cols = _band(n, 4, rng)
        pals = _disjoint_palettes([k0] + [512] * 7, rng)
        out.append(Case(name, *_csr(n, rows, cols, _tile_values(n, rows, pals, rng)),
                        {"nnz": 16384, "tile_total": 4096 + (k0 - 512), "distinct": 4096 + (k0 - 512)}))
    return out


def _packing_cases():
    out = []
    for n in (1 << 21, (1 << 21) + 1):   # 2048 values: 21 + 11 = 32 bits (packed), 22 + 11 (windowed columns)
        rng = np.random.default_rng(300 + n)
        rows = np.repeat(np.arange(n, dtype=np.int64), 2)
        cols = rows.copy()
        cols[1::2] = (np.arange(n) + 1) % n
        out.append(Case(f"pack_2048_n{n}", *_csr(n, rows, cols, _cover(len(rows), _palette(2048, rng), rng)),
                        {"n": n, "distinct": 2048}, spd=False))
    return out


def _window_cases():
    """tile 0 touches exactly 64 / 65 windows of 2^14 ids; the 65th is the last, partial window of the id range"""
    out = []
    n = 64 * (1 << WIN_BITS) + 1000
    for many_values in (False, True):
        for nwin in (64, 65):
            rng = np.random.default_rng(400 + nwin + 10 * many_values)
            rows = [np.arange(n, dtype=np.int64)]
            cols = [np.arange(n, dtype=np.int64)]
            w = np.arange(1, 64)                  # row w of tile 0 reads window w (window 0: the diagonal)
            rows.append(w)
            cols.append((w << WIN_BITS) + np.where(w % 2 == 0, 0, (1 << WIN_BITS) - 1))   # offsets 0 and 2^14 - 1
            if nwin == 65:
                rows.append(np.array([64]))
                cols.append(np.array([n - 1]))     # window 64: the last, partial one
            rows, cols = np.concatenate(rows), np.concatenate(cols)
            if many_values:   # 3000 values, 64 per tile: tile-local dictionaries
                pal = _palette(3000, rng)
                ntiles = (n + TILE_ROWS - 1) // TILE_ROWS
                pals = [pal[(23 * t + np.arange(64)) % 3000] for t in range(ntiles)]
                pals[-1] = pals[-1][:min(64, n - (ntiles - 1) * TILE_ROWS)]
                vals = _tile_values(n, rows, pals, rng)
            else:
                vals = _cover(len(rows), _palette(8, rng), rng)
            name = f"win_{nwin}" + ("_tiles" if many_values else "")
            out.append(Case(name, *_csr(n, rows, cols, vals),
                            {"tile_windows": {0: nwin, 1: 1}, "tile_offsets": {0: [0, (1 << WIN_BITS) - 1]},
                             "last_window_partial": nwin == 65, **({"distinct": 3000} if many_values else {})}))
    return out


def _geometry_cases():
    out = []
    for n in (1, 3, 511, 512, 513):
        rng = np.random.default_rng(500 + n)
        lens = rng.integers(1, 7, n)
        rows = np.repeat(np.arange(n, dtype=np.int64), lens)
        cols = rng.integers(0, n, len(rows))
        out.append(Case(f"n_{n}", *_csr(n, rows, cols, _cover(len(rows), _palette(min(5, len(rows)), rng), rng)), {"n": n}, f32=True))

    # tile t starts at row_ptr = t (mod 4): every alignment of the first code / column quad
    rng = np.random.default_rng(510)
    n = 8 * TILE_ROWS
    lens = rng.integers(3, 8, n)
    for t in range(1, 8):
        r = t * TILE_ROWS - 1                       # the last row of tile t - 1 sets where tile t starts
        lens[r] += (t % 4 - int(lens[:r + 1].sum()) % 4) % 4
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = rng.integers(0, n, len(rows))
    out.append(Case("head_mod4", *_csr(n, rows, cols, _cover(len(rows), _palette(6, rng), rng)),
                    {"tile_head_mod4": {t: t % 4 for t in range(8)}}, f32=True))

    # a tile with one pass less one, one pass, one pass and one product (tile 0 holds 1001 entries: tile 1 starts at 1 mod 4)
    for k in (4095, 4096, 4097):
        rng = np.random.default_rng(520 + k)
        n = 3 * TILE_ROWS
        lens = np.full(n, 3)
        lens[:TILE_ROWS] = 1001 // TILE_ROWS
        lens[:1001 % TILE_ROWS] += 1
        lens[TILE_ROWS:2 * TILE_ROWS] = k // TILE_ROWS
        lens[TILE_ROWS:TILE_ROWS + k % TILE_ROWS] += 1
        rows = np.repeat(np.arange(n, dtype=np.int64), lens)
        cols = rng.integers(0, n, len(rows))
        out.append(Case(f"tile_nnz_{k}", *_csr(n, rows, cols, _cover(len(rows), _palette(7, rng), rng)),
                        {"tile_nnz": {0: 1001, 1: k}}, f32=(k == 4097)))

    # one row of 10,000 entries (three passes), unsorted, with repeated columns
    rng = np.random.default_rng(530)
    n = 1500
    lens = np.full(n, 3)
    lens[700] = 10000
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = rng.integers(0, n, len(rows))
    out.append(Case("long_row", *_csr(n, rows, cols, _cover(len(rows), _palette(9, rng), rng)), {"longest_row": 10000}, f32=True))

    # empty rows and an empty tile: tile 1 has no entries, every 7th row is empty, so are the last five rows
    rng = np.random.default_rng(540)
    n = 4 * TILE_ROWS + 100
    lens = rng.integers(1, 6, n)
    lens[TILE_ROWS:2 * TILE_ROWS] = 0
    lens[::7] = 0
    lens[-5:] = 0
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = rng.integers(0, n, len(rows))
    out.append(Case("empty_rows", *_csr(n, rows, cols, _cover(len(rows), _palette(4, rng), rng)),
                    {"empty_tiles": [1], "empty_rows_at_least": n // 7 + 5}, f32=True))

    # columns just inside and just outside the tile's x window [row0, row0 + 512)
    rng = np.random.default_rng(550)
    n = 5 * TILE_ROWS + 37
    rows, cols = [], []
    for t in range((n + TILE_ROWS - 1) // TILE_ROWS):
        row0 = t * TILE_ROWS
        for j, c in enumerate((row0 - 1, row0, row0 + TILE_ROWS - 1, row0 + TILE_ROWS)):
            if 0 <= c < n:
                rows.append(row0 + 3 * j)
                cols.append(c)
    rows = np.concatenate([np.array(rows), np.arange(n)])
    cols = np.concatenate([np.array(cols), np.arange(n)])
    out.append(Case("x_window_edges", *_csr(n, rows, cols, _cover(len(rows), _palette(5, rng), rng)),
                    {"x_window_cols": {0: [0, 511, 512], 1: [-1, 0, 511, 512], 4: [-1, 0, 511, 512], 5: [-1, 0]}}, f32=True))
    return out


def _value_cases():
    out = []
    rng = np.random.default_rng(600)
    n = 600
    special = np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308 / 3, 1e300, -1e300, 1e-300, np.inf, -np.inf, np.nan, 0.5, 2.0])
    rows, cols = _band(n, 5, rng, width=20)
    out.append(Case("specials", *_csr(n, rows, cols, _cover(len(rows), special, rng)),
                    {"bit_patterns": [int(b) for b in special.view(np.uint64)]}, spd=False))

    rng = np.random.default_rng(610)
    n = 3000
    lens = rng.integers(4, 9, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = rng.integers(0, n, len(rows))
    cols[1::3] = cols[0::3][:len(cols[1::3])]      # repeats inside a row (and across row boundaries now and then)
    out.append(Case("unsorted_repeated", *_csr(n, rows, cols, _cover(len(rows), _palette(10, rng), rng)),
                    {"unsorted_rows": True, "repeated_columns": True}, f32=True))

    rng = np.random.default_rng(620)
    n = 20000
    rows = np.repeat(np.arange(n, dtype=np.int64), 6)
    cols = rng.integers(0, n, len(rows))
    cols[0], cols[-1] = n - 1, 0
    out.append(Case("random_cols", *_csr(n, rows, cols, _cover(len(rows), _palette(12, rng), rng)), {"column_span": [0, n - 1]}))

    # one entry with the bit pattern of the hash tables' empty key
    rng = np.random.default_rng(630)
    n = 2000
    rows, cols = _band(n, 4, rng)
    r, c, v = _csr(n, rows, cols, _cover(len(rows), _palette(4, rng), rng))
    v.view(np.uint64)[777] = np.uint64(EMPTY_BITS)
    out.append(Case("sentinel", r, c, v, {"bit_patterns": [EMPTY_BITS]}, spd=False))
    return out


NAMES = ["dist_1", "dist_2048", "dist_2049", "dist_65536_n65536", "dist_65536_n65537", "dist_65537",
         "tile_1024", "tile_1025", "tile_3072", "tile_3073", "quarter_in", "quarter_out",
         "pack_2048_n2097152", "pack_2048_n2097153",
         "win_64", "win_65", "win_64_tiles", "win_65_tiles",
         "n_1", "n_3", "n_511", "n_512", "n_513", "head_mod4", "tile_nnz_4095", "tile_nnz_4096", "tile_nnz_4097", "long_row",
         "empty_rows", "x_window_edges",
         "specials", "unsorted_repeated", "random_cols", "sentinel"]
SPD_NAMES = [n for n in NAMES if not n.startswith("pack_") and n not in ("specials", "sentinel")]   # (Case.spd)


def cases():
    """every named case (about 6 M non-zeros in all; the two 2^21-row packing cases are most of it)"""
    return _distinct_cases() + _tile_cases() + _packing_cases() + _window_cases() + _geometry_cases() + _value_cases()


def spd_version(case, seed=0):
    """(row_ptr, col, val, b): the case's pattern made symmetric, off-diagonal entries -|v| from the case's values (< 1 in magnitude),
    the diagonal = 1 + number of off-diagonal entries of the row -- strictly diagonally dominant, columns sorted, no repeats"""
    rp = case.row_ptr.astype(np.int64)
    n = case.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = case.col.astype(np.int64)
    off = rows != cols
    a, b = np.minimum(rows[off], cols[off]), np.maximum(rows[off], cols[off])
    _, first = np.unique(a * n + b, return_index=True)
    a, b, w = a[first], b[first], -np.abs(case.val[off][first])
    assert np.all(np.abs(w) < 1.0)
    r2 = np.concatenate([a, b, np.arange(n)])
    c2 = np.concatenate([b, a, np.arange(n)])
    m = np.bincount(np.concatenate([a, b]), minlength=n)
    v2 = np.concatenate([w, w, 1.0 + m])
    order = np.lexsort((c2, r2))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(r2, minlength=n))
    rhs = np.random.default_rng(seed).standard_normal(n)
    return row_ptr.astype(np.int32), c2[order].astype(np.int32), v2[order], rhs
