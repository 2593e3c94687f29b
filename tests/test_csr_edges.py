"""The CSR edge cases of tests/csr_edges.py are what their names say, and the restated form rule reaches every storage form.

The properties are counted here with plain Python sets and loops over the arrays, not through `expected_format` (the rule the GPU tests
compare the library with)."""
import numpy as np
import pytest

import csr_edges as E

CASES = {c.name: c for c in E.cases()}


def _tile_span(c, t):
    r0 = t * E.TILE_ROWS
    r1 = min(r0 + E.TILE_ROWS, c.n)
    return int(c.row_ptr[r0]), int(c.row_ptr[r1])


def _tile_set(c, t, arr):
    s, e = _tile_span(c, t)
    return set(arr[s:e].tolist())


def _ntiles(c):
    return (c.n + E.TILE_ROWS - 1) // E.TILE_ROWS


def _check(c, key, want):
    bits = c.val.view(np.uint64)
    if key == "n":
        assert c.n == want
    elif key == "nnz":
        assert int(c.row_ptr[-1]) == want
    elif key == "distinct":
        assert len(set(bits.tolist())) == want
    elif key == "max_tile_distinct":
        assert max(len(_tile_set(c, t, bits)) for t in range(_ntiles(c))) == want
    elif key == "tile_distinct":
        for t, k in want.items():
            assert len(_tile_set(c, t, bits)) == k, t
    elif key == "tile_total":
        assert sum(len(_tile_set(c, t, bits)) for t in range(_ntiles(c))) == want
    elif key == "tile_total_over_quarter":
        total = sum(len(_tile_set(c, t, bits)) for t in range(_ntiles(c)))
        assert (8 * total > 2 * int(c.row_ptr[-1])) == want
    elif key == "tile_windows":
        for t, k in want.items():
            assert len({v // (1 << E.WIN_BITS) for v in _tile_set(c, t, c.col)}) == k, t
    elif key == "tile_offsets":
        for t, offs in want.items():
            assert set(offs) <= {v % (1 << E.WIN_BITS) for v in _tile_set(c, t, c.col)}, t
    elif key == "last_window_partial":
        last = (c.n - 1) // (1 << E.WIN_BITS)
        assert c.n % (1 << E.WIN_BITS) != 0
        assert any(v // (1 << E.WIN_BITS) == last for v in _tile_set(c, 0, c.col)) == want
    elif key == "tile_head_mod4":
        for t, r in want.items():
            assert int(c.row_ptr[t * E.TILE_ROWS]) % 4 == r, t
    elif key == "tile_nnz":
        for t, k in want.items():
            s, e = _tile_span(c, t)
            assert e - s == k, t
    elif key == "longest_row":
        assert max(int(c.row_ptr[i + 1]) - int(c.row_ptr[i]) for i in range(c.n)) == want
    elif key == "empty_tiles":
        for t in want:
            s, e = _tile_span(c, t)
            assert s == e, t
    elif key == "empty_rows_at_least":
        assert sum(1 for i in range(c.n) if c.row_ptr[i + 1] == c.row_ptr[i]) >= want
        assert c.row_ptr[-1] == c.row_ptr[-6]              # the last five rows
    elif key == "x_window_cols":
        for t, offs in want.items():
            row0 = t * E.TILE_ROWS
            assert set(offs) <= {v - row0 for v in _tile_set(c, t, c.col)}, t
    elif key == "bit_patterns":
        assert set(want) <= set(bits.tolist())
    elif key in ("unsorted_rows", "repeated_columns"):
        rows = [c.col[c.row_ptr[i]:c.row_ptr[i + 1]].tolist() for i in range(c.n)]
        if key == "unsorted_rows":
            assert any(r != sorted(r) for r in rows) == want
        else:
            assert any(len(set(r)) < len(r) for r in rows) == want
    elif key == "column_span":
        assert [int(c.col.min()), int(c.col.max())] == want
    else:
        raise AssertionError(f"unknown property {key}")


@pytest.mark.parametrize("name", list(CASES))
def test_case_has_its_named_property(name):
    c = CASES[name]
    assert c.props, "every case names what it is for"
    assert c.row_ptr[0] == 0 and np.all(np.diff(c.row_ptr) >= 0) and c.row_ptr[-1] == len(c.col) == len(c.val)
    assert c.n <= 2_200_000 and (c.n == 0 or (c.col.min() >= 0 and c.col.max() < c.n))
    for key, want in c.props.items():
        _check(c, key, want)


def test_name_lists_match_the_cases():
    assert list(CASES) == E.NAMES
    assert [c.name for c in CASES.values() if c.spd] == E.SPD_NAMES


def test_cases_are_reproducible():
    again = {c.name: c for c in E.cases()}
    for name, c in CASES.items():
        d = again[name]
        assert np.array_equal(c.row_ptr, d.row_ptr) and np.array_equal(c.col, d.col)
        assert np.array_equal(c.val.view(np.uint64), d.val.view(np.uint64))


def test_bits_for():
    assert [E.bits_for(k) for k in (1, 2, 3, 2048, 2049, 65536, 65537, 1 << 21, (1 << 21) + 1)] == [1, 1, 2, 11, 12, 16, 17, 21, 22]


# what the default environment must give the cases on either side of a threshold
DEFAULT_FORM = {
    "dist_1": "LDS dictionary packed",
    "dist_2048": "LDS dictionary packed",
    "dist_2049": "tile dictionary windowed",
    "dist_65536_n65536": "L1 dictionary packed",
    "dist_65536_n65537": "L1 dictionary 6 B",
    "dist_65537": "plain CSR",
    "tile_1024": "tile dictionary windowed",
    "tile_1025": "tile dictionary windowed + big",
    "tile_3072": "tile dictionary windowed + big",
    "tile_3073": "L1 dictionary packed",
    "quarter_in": "tile dictionary windowed",
    "quarter_out": "L1 dictionary packed",
    "pack_2048_n2097152": "LDS dictionary packed",
    "pack_2048_n2097153": "LDS dictionary windowed",
    "win_64": "LDS dictionary packed",
    "win_64_tiles": "tile dictionary windowed",
    "win_65_tiles": "tile dictionary 6 B",
    "sentinel": "plain CSR",
}


@pytest.mark.parametrize("name", list(DEFAULT_FORM))
def test_rule_puts_the_threshold_cases_on_their_side(name):
    c = CASES[name]
    assert E.instantiation(E.expected_format(c.row_ptr, c.col, c.val), c.row_ptr, c.val) == DEFAULT_FORM[name]


def test_rule_reaches_every_form():
    """Over all cases and environments the rule (and so the GPU tests, which assert it) reaches every instantiation of the table."""
    reached = set()
    for c in CASES.values():
        for env in E.ENVS.values():
            reached.add(E.instantiation(E.expected_format(c.row_ptr, c.col, c.val, env), c.row_ptr, c.val))
    want = {"LDS dictionary packed", "LDS dictionary windowed", "LDS dictionary 6 B", "tile dictionary windowed", "tile dictionary 6 B",
            "tile dictionary windowed + big", "tile dictionary 6 B + big", "L1 dictionary packed", "L1 dictionary 6 B", "plain CSR"}
    assert want <= reached, want - reached


def test_rule_on_the_windows_and_the_sentinel():
    c = CASES["win_65"]
    assert E.instantiation(E.expected_format(c.row_ptr, c.col, c.val, E.ENVS["no_pack"])) == "LDS dictionary 6 B"
    c = CASES["win_64"]
    assert E.instantiation(E.expected_format(c.row_ptr, c.col, c.val, E.ENVS["no_pack"])) == "LDS dictionary windowed"
    c = CASES["sentinel"]
    for env in E.ENVS.values():
        assert E.expected_format(c.row_ptr, c.col, c.val, env)["bytes_per_nonzero"] == 12


def test_spd_versions_are_symmetric_and_dominant():
    for c in CASES.values():
        if not c.spd or c.n > 100_000:
            continue
        rp, col, val, b = E.spd_version(c)
        rows = np.repeat(np.arange(c.n), np.diff(rp))
        dense = {}
        for i, j, v in zip(rows.tolist(), col.tolist(), val.tolist()):
            assert (i, j) not in dense
            dense[(i, j)] = v
        diag = np.zeros(c.n)
        off = np.zeros(c.n)
        for (i, j), v in dense.items():
            assert dense.get((j, i)) == v
            if i == j:
                diag[i] = v
            else:
                off[i] += abs(v)
        assert np.all(diag > off), c.name
