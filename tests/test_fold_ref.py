"""The fold and compaction KAT without a GPU: tests/fold_ref.py's speculative window held
to tests/adaptive_spec_ref.py's pass loop, and the preconditions of every case of
tests/test_device_fold_kat.py, shown from the restatement alone on the seeded inputs."""
import numpy as np
import pytest

import adaptive_resume_ref as rr
import adaptive_spec_ref as sr
import fold_ref as fr

F = np.float32


# ---------------------------------------------------------------- the chaining identity
# 200 slots, budget 30, batch 4, passes of up to 12 samples: 0..12, 12..24 and 24..30, whose
# end is off the batch grid.  Window widths aligned with the batch (4, 8, 12) and not (5, 7).
CHAIN = dict(budget=30, batch_spp=4, min_spp=8, rel_tol=0.05, abs_eps=1e-3)


@pytest.fixture(scope="module")
def chain_pass_loop():
    paths = fr.samples(41, 200, CHAIN["budget"])
    st, log = sr.resume(paths, rr.zero_state(200), CHAIN["budget"], CHAIN["batch_spp"], CHAIN["min_spp"],
                        CHAIN["rel_tol"], CHAIN["abs_eps"], 12, sr.HUGE)
    assert [(e["level"], e["w"]) for e in log] == [(0, 12), (12, 12), (24, 6)]
    assert all(e["discarded"] > 0 for e in log[:2]) and log[1]["active"].size < 200
    return paths, st, log


@pytest.mark.parametrize("width", (4, 5, 7, 8, 12))
def test_chained_windows_leave_the_pass_loops_state(chain_pass_loop, width):
    paths, want, log = chain_pass_loop
    st = fr.new_state(200, seed=42)  # garbage: a slot without samples starts from zero
    for e in log:
        act = e["active"].astype(np.int32)
        sample = np.ascontiguousarray(paths[act, e["level"]:e["level"] + e["w"]])
        st, keep, ctr, _ = fr.spec_pass(sample, st, act, width, n=e["level"], **CHAIN)
        np.testing.assert_array_equal(st["count"][act], e["stop"])
        assert int(ctr[0]) == e["discarded"]
        np.testing.assert_array_equal(keep, (e["stop"] == e["level"] + e["w"]) &
                                      ~rr.retired(dict(count=st["count"][act], s1=st["mom"][act, 0].copy(),
                                                       s2=st["mom"][act, 1].copy()), CHAIN["budget"], CHAIN["min_spp"],
                                                  CHAIN["rel_tol"], CHAIN["abs_eps"]))
    sr.same_state(dict(count=st["count"], s1=st["mom"][:, 0].copy(), s2=st["mom"][:, 1].copy()), want)


# ---------------------------------------------------------------- the speculative cases
def facts_of(name, width):
    c = fr.spec_case(name)
    st, keep, ctr, facts = fr.spec_pass(c["sample"], c["state"], c["active_slot"], width, **c["rule"])
    return c, st, keep, ctr, facts, fr.window_plan(c["sample"].shape[1], width)


@pytest.mark.parametrize("width", fr.SPEC_WIDTHS)
@pytest.mark.parametrize("name", ("fresh", "resumed"))
def test_a_speculative_case_holds_what_it_is_named_for(name, width):
    c, st, keep, ctr, facts, plan = facts_of(name, width)
    n, batch = c["rule"]["n"], c["rule"]["batch_spp"]
    rows = c["sample"].shape[0]
    assert rows % 256 not in (0, 255) and rows > 256  # a partial last block
    later = [f for (s0, _), f in zip(plan, facts) if s0 > 0]
    # a slot that stopped in an earlier window, told by its count ("fresh" at 20 has two windows,
    # and nothing stops in its first)
    assert sum(f["mismatch"] for f in later) > 0 or (name, width) == ("fresh", 20)
    # a stop strictly inside a 16-sample chunk
    assert sum(f["inside"] for f in facts) > 0
    # the pass ends off the batch grid, and slots stop there
    assert c["sample"].shape[1] % batch != 0 and facts[-1]["end_off_grid"] > 0
    # the counters: fewer stops below the budget than rows not kept, in one window
    if name == "fresh":
        assert facts[0]["stops"] == 0 and facts[0]["kept"] == rows  # a window in which nothing stops
        assert facts[-1]["budget"] > 0 and int(ctr[1]) < int((keep == 0).sum())
    else:
        assert all(f["budget"] == 0 for f in facts) and (keep == 1).any()
    assert int(ctr[0]) > 0 and int(ctr[1]) > 0


@pytest.mark.parametrize("name", ("fresh", "resumed"))
def test_a_speculative_case_over_its_widths(name):
    """What only some widths can hold: a window base on the batch grid at which a slot has just
    retired (its count equals the base), and a base off the grid at which the rule holds for a
    slot that goes on, since nothing asked (folded; a kernel that asked there would drop it);
    and, in the case that reaches its budget, a window with stops by budget and by rule."""
    at_base, plain, both = {}, {}, {}
    for width in fr.SPEC_WIDTHS:
        facts = facts_of(name, width)[4]
        both[width] = any(f["budget"] > 0 and f["rule"] > 0 for f in facts)
        at_base[width] = sum(f["at_base"] for f in facts)
        plain[width] = sum(f["rule_at_plain_base"] for f in facts)
    assert any(at_base[k] > 0 for k in (12, 16, 20)), at_base                # 16-byte loads
    assert any(at_base[k] > 0 for k in (6, 14, 18)), at_base                 # scalar loads
    assert any(plain[k] > 0 for k in (6, 14, 18)), plain
    if name == "fresh":  # stops by budget and by rule in one window
        assert any(both[k] for k in (12, 16, 20)) and any(both[k] for k in (6, 14, 18)), both


# ---------------------------------------------------------------- the ordering inputs
@pytest.mark.parametrize("rows", (257, 513))
def test_the_order_of_additions_shows_in_the_inputs(rows):
    rev, chunked = fr.order_shares(fr.samples(rows, rows, fr.ORDER_SPP, nan=True))
    assert rev >= fr.ORDER_MIN_SHARE and chunked >= fr.ORDER_MIN_SHARE, (rev, chunked)


def test_the_generator_holds_every_kind_of_value():
    x = fr.samples(7, 513, 36)
    assert not np.isnan(x).any() and np.isnan(fr.samples(7, 513, 36, nan=True)).any()
    assert (x == np.inf).any() and (x == -np.inf).any() and (x < 0).any()
    assert ((x == 0) & ~np.signbit(x)).any() and ((x == 0) & np.signbit(x)).any()
    fin = np.abs(x[np.isfinite(x) & (x != 0)])
    assert fin.max() > 2.0 ** 25 and fin.min() < 2.0 ** -60
    # rows whose second moment passes through denormals on its way
    st, _ = fr.adaptive_fold(x, fr.new_state(513), np.zeros(513, np.uint8), init=1)
    s2 = st["mom"][:, 1]
    assert ((s2 > 0) & (s2 < np.finfo(F).tiny)).sum() >= 5
    assert np.isnan(st["mom"]).any()  # Inf - Inf, without a NaN among the samples


# ---------------------------------------------------------------- level, select, finish
@pytest.mark.parametrize("n_slots", fr.LEVEL_SLOTS)
def test_the_level_cases(n_slots):
    out = {k: fr.level_finish(**fr.level_case(k, n_slots), **fr.LEVEL_RULE) for k in fr.LEVEL_CASES}
    assert out["retired"]["n_live"] == 0 and out["retired"]["level"] == fr.INT_MAX and not out["retired"]["keep"].any()
    assert out["one_level"]["n_live"] == n_slots and out["one_level"]["level"] == 8 and out["one_level"]["keep"].all()
    if n_slots < 255:
        return
    c, o = fr.level_case("levels", n_slots), out["levels"]
    live = o["live"] != 0
    assert o["level"] == 0 and np.unique(c["count"][live]).size >= 3 and 0 < o["keep"].sum() < o["n_live"] < n_slots
    assert 0 < o["below"] < n_slots
    nan = np.isnan(c["mom"]).any(axis=1) & (c["count"] >= 8) & (c["count"] < 16)
    assert nan.any() and live[nan].all()  # a NaN moment never converges
    neg = (c["mom"][:, 0] == 10) & (c["count"] >= 8) & (c["count"] < 16)
    assert neg.any() and not live[neg].any()  # a negative variance does
    assert (o["mean"][c["count"] == 0] == 0).all() and np.isnan(c["sums"][c["count"] == 0]).any()


# ---------------------------------------------------------------- compaction
def test_the_compaction_cases():
    n = fr.COMPACT_ROWS[-1]
    assert n == 2 * fr.SCAN_CHUNK + 1 and fr.COMPACT_ROWS[-3:-1] == (fr.SCAN_CHUNK, fr.SCAN_CHUNK + 1)
    keep = fr.compact_keep("third_chunk", n)
    assert keep[2 * fr.SCAN_CHUNK] == 1 and keep[:fr.SCAN_CHUNK].sum() > 256 and keep[fr.SCAN_CHUNK:2 * fr.SCAN_CHUNK].sum() > 256
    assert all(fr.compact_keep("third_chunk", k) is None for k in fr.COMPACT_ROWS[:-1])
    assert set(np.unique(fr.compact_keep("bytes", 257))) == {0, 1, 2, 255}
    k = fr.compact_keep("p50", 257)  # survivors in every wave of both blocks, and gaps between them
    assert all(0 < k[a:a + 64].sum() < 64 for a in (0, 64, 128, 192)) and k[256] in (0, 1)
    slot, pix = fr.compact(k, np.arange(300, 300 - 257, -1, dtype=np.int32), np.arange(1000, dtype=np.int32)[::-1].copy())
    np.testing.assert_array_equal(slot, 300 - np.flatnonzero(k))
    np.testing.assert_array_equal(pix, 999 - slot)


# ---------------------------------------------------------------- the emission counts
@pytest.mark.parametrize("s0,spp_b,ns", ((0, 4, 8), (4, 4, 8), (7, 7, 20)))
def test_the_emission_counts_hold_every_class(s0, spp_b, ns):
    ni = np.clip(fr.emission_counts(64, ns, s0, spp_b), 1, ns)
    assert (fr.emission_counts(64, ns, s0, spp_b) <= 0).any() and (fr.emission_counts(64, ns, s0, spp_b) > ns).any()
    if s0 > 0:
        assert (ni <= s0).any()                          # ended in an earlier batch
    assert (ni == s0 + spp_b).any()                      # ends with the batch
    assert (ni > s0 + spp_b).any() or s0 + spp_b == ns   # goes on
    if spp_b > 2:
        assert ((ni > s0 + 1) & (ni < s0 + spp_b)).any()  # ends strictly inside


def test_the_mean_factor_is_the_double_division_rounded_once():
    for n in (1, 3, 7, 344, 1024, 16777216):
        assert fr.inv(n) == F(1.0 / float(n)) and fr.inv_many(np.array([n]))[0] == fr.inv(n)
