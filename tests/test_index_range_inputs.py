"""The CPU companion of tests/test_gpu_index_range.py: what that file's rows claim, checked without a GPU.

For every row of tests/index_range.py: the sample indices are the ones its table says (the straddles of 2^31 and the +Inf / signalling NaN
/ quiet NaN / sign-bit bands of the float whose bits the index is), the frame is one the entry points accept, the fp64 restatement alone
is finite there, reaches every parameter that requires a gradient, caps no path and leaves every other image row exactly zero, and the
recorded seed is one at which the restatement calls the row stable (tests/f32_flips.py's stand-in criterion and the conditioning rule of
tests/test_gpu_launch_geometry.py) -- so no seed is in the table by hand."""
import numpy as np
import pytest

import f32_flips as ff
import index_range as ir

ALL_ROWS = list(ir.ROWS)
ids = lambda rows: [f"{f}-{r}" for f, r in rows]


@pytest.mark.parametrize("where", ALL_ROWS, ids=ids(ALL_ROWS))
def test_the_rows_are_where_the_table_says(where):
    frame, row = where
    w, h, spp, limit = ir.FRAMES[frame]
    first, last, _ = ir.ROWS[where]
    assert w * h * spp <= limit
    assert ir.interval(w, h, spp, row) == (first, last) and last - first + 1 == ir.row_paths(where)
    assert 0 <= first <= last <= 2 ** 32 - 1
    assert ir.patterns_between(first, last) == ir.ROW_PATTERNS[where]
    assert ir.pattern_of(first) == ir.ROW_PATTERNS[where][0] and ir.pattern_of(last) == ir.ROW_PATTERNS[where][-1]
    # the float whose bits are the index really is what the band's name says
    as_float = np.array([first, last], np.uint32).view(np.float32)
    for v, name in zip(as_float, (ir.pattern_of(first), ir.pattern_of(last))):
        assert np.isnan(v) == ("NaN" in name) and np.isinf(v) == ("Inf" in name)
        assert bool(np.signbit(v)) == name.startswith(("-", "negative"))


def test_the_frames_and_their_edges():
    w, h, spp, _ = ir.FRAMES["top"]
    assert w * h * spp == 2 ** 32 and w * h * (spp + 1) > 2 ** 32 and 65536 * 65536 * 2 > 2 ** 32
    assert ir.ROWS[("top", 8160)][0] == 0x7F800000 and ir.ROWS[("top", 8191)][1] == 0x7FFFFFFF
    assert ir.ROWS[("top", 8192)][0] == 0x80000000 and ir.ROWS[("top", 16383)][1] == 0xFFFFFFFF
    assert ir.ROWS[("top", 8160)][1] < 0x7FC00000 <= ir.ROWS[("top", 8191)][0]             # all signalling; all quiet
    assert ir.ROWS[("top", 16383)][0] > 0xFF800000
    # `odd`: 2^31 falls inside the samples of pixel 29 of the row (global pixel 715589) -- lane 29 of a wave of 64, not at a sample range's edge
    w, h, spp, _ = ir.FRAMES["odd"]
    assert w * h * spp == 4294911160 and all(v % 2 for v in (h, spp))
    first, last, _ = ir.ROWS[("odd", 17889)]
    assert first < 2 ** 31 < last and 2 ** 31 // spp == 715589 == 17889 * w + 29 and 0 < 2 ** 31 % spp < spp - 1
    # `half`: the largest frame of its shape the derived forms accept
    w, h, spp, limit = ir.FRAMES["half"]
    assert w * h * spp == 2146959360 <= limit == 2 ** 31 - 1 < w * h * (spp + 1)
    # three rows in one shard: 2^31 is the first sample of a pixel that starts a group of 64
    b = ir.BAND3
    w, h, spp, _ = ir.FRAMES[b["frame"]]
    rows = [y for y in range(h) if (y // b["band_rows"]) % b["n_shards"] == b["shard"]]
    assert tuple(rows) == b["rows"] and ir.interval(w, h, spp, rows[0], 3)[0] < 2 ** 31 < ir.interval(w, h, spp, rows[0], 3)[1]
    assert 2 ** 31 % spp == 0 and ((2 ** 31 // spp) - rows[0] * w) % 64 == 0
    e = ir.EMPTY_SHARD
    assert not [y for y in range(ir.FRAMES[e["frame"]][1]) if (y // e["band_rows"]) % e["n_shards"] == e["shard"]]
    assert set(ir.SEEDS) <= {(f,) + w for f in ir.FAMILIES for w in ir.ROWS} and not any(k[0] in ir.F64_ONLY for k in ir.SEEDS)


FAMILY_ROWS = [(f, w) for f in ir.FAMILIES for w in ir.RENDER_ROWS] + [("depth4", ir.HALF_ROW)]


@pytest.mark.parametrize("family,where", FAMILY_ROWS, ids=[f"{f}-{w[0]}-{w[1]}" for f, w in FAMILY_ROWS])
def test_the_restatement_alone(pkg, oracle, family, where):
    """finite, every parameter that requires a gradient reached, no path capped (deepest < 64), every other image row exactly zero -- under
    the unbiased operator too where a case uses it"""
    x = ir.inputs(pkg, family, where)
    for what in ("bwd",) + (("unbiased",) if family in ir.UNBIASED else ()):
        r = ir.expected(oracle, x, what)
        own, others_zero = ir.row_of(r["image"], where)
        assert others_zero and own.any() and np.isfinite(r["image"]).all() and np.isfinite(r["grads"]).all()
        assert all(r["grads"][p].any() for p in ff.wanted(x.scene)), [p for p in ff.wanted(x.scene) if not r["grads"][p].any()]
        assert r["stats"]["paths"] == ir.row_paths(where) and r["stats"]["deepest"] < 64 and r["stats"]["extreme_draws"] == 0


STABLE_ROWS = [(f, w) for f, w in FAMILY_ROWS if f not in ir.F64_ONLY]


@pytest.mark.parametrize("family,where", STABLE_ROWS, ids=[f"{f}-{w[0]}-{w[1]}" for f, w in STABLE_ROWS])
def test_every_row_is_stable_at_its_recorded_seed(pkg, oracle, family, where):
    ok, rec = ir.stable_record(oracle, ir.inputs(pkg, family, where))
    assert ok, rec


@pytest.mark.parametrize("family", ir.F64_ONLY)
def test_the_f64_only_families_are_not_stable(pkg, oracle, family):
    """(at the first seed of the control row and of the last row; tests/index_range.py says what rejects them at all of 1 ... SEED_LIMIT)"""
    for where in (("top", 0), ir.TOP_LAST):
        ok, rec = ir.stable_record(oracle, ir.inputs(pkg, family, where))
        assert not ok, rec
