"""The kernels that turn samples into pixels restated in numpy float32, one function per
kind of srr_device_fold_kat (include/srr_capi.h), written from the contracts in
csrc/kernels.h (launch_accumulate_window, AdaptiveFold, AdaptiveSpecFold, AdaptiveRule,
launch_adaptive_compact, AovFold, AovEmissionFold) and not from the kernels.  A sum is one
float32 addition per sample in sample order; a mean is sum * (float)(1.0 / (float)n).  The
convergence rule and the retirement are tests/adaptive_ref.py's and
tests/adaptive_resume_ref.py's.  Also here: the seeded sample generator and the cases that
tests/test_fold_ref.py (CPU: their preconditions) and tests/test_device_fold_kat.py (GPU)
share.  Every function returns new arrays and leaves its arguments alone."""
from __future__ import annotations

import functools

import numpy as np

import adaptive_ref as ar
import adaptive_resume_ref as rr

F = np.float32
INT_MAX = 2**31 - 1
CHUNK = 16  # samples a block stages at a time (kernels.hip kAccChunk)


def inv(n) -> np.float32:
    """(float)(1.0 / (float)n): the division in double, rounded once to float32."""
    return F(np.float64(1.0) / np.float64(F(n)))


def inv_many(n: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (np.float64(1.0) / n.astype(F).astype(np.float64)).astype(F)


def ordered_sum(start: np.ndarray, x: np.ndarray) -> np.ndarray:
    """start[rows, ...] + x[rows, 0, ...] + x[rows, 1, ...] + ..., one float32 addition each."""
    s = start.astype(F, copy=True)
    assert x.dtype == F
    with np.errstate(all="ignore"):
        for k in range(x.shape[1]):
            s = s + x[:, k]
    assert s.dtype == F
    return s


def same_bits(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """Bitwise equality of float32 arrays; where `want` is NaN, `got` must be NaN (any payload)."""
    assert got.dtype == F and want.dtype == F and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN places")
    np.testing.assert_array_equal(np.where(nan, F(0), got).view(np.uint32), np.where(nan, F(0), want).view(np.uint32),
                                  err_msg=f"{what}: bits")


# ---------------------------------------------------------------- the sample generator
def samples(seed: int, rows: int, spp: int, words: int = 3, nan: bool = False) -> np.ndarray:
    """float32 [rows, spp, words].  Rows are of four sorts, dealt at random: calm (a row
    colour times 1 + a * (u - 0.5), the row's a spread over 0.1 .. 3: these decide the
    convergence rule at different counts), uniform [0, 1), wild (sign * 2^u, u uniform in
    -30 .. 30: addition order decides the low bits), and tiny (uniform * 2^-66: the squares
    of their luminances are denormal).  Over the rows that are not calm, elements become
    negative, 0, -0.0 and (rarely) +-Inf; with `nan`, a few NaN go anywhere."""
    r = np.random.default_rng(seed)
    shape = (rows, spp, words)
    u = r.random(shape, dtype=F)
    sort = r.choice(4, size=rows, p=[0.45, 0.2, 0.25, 0.1])
    if rows >= 4:  # every sort is present
        sort[r.choice(rows, size=4, replace=False)] = np.arange(4)
    out = u.copy()
    calm = sort == 0
    amp = (F(0.1) * F(30.0) ** r.random(rows, dtype=F))[:, None, None]
    colour = (F(0.05) + r.random((rows, 1, words), dtype=F))
    out[calm] = (colour * (F(1) + amp * (u - F(0.5))))[calm]
    wild = sort == 2
    mag = np.exp2(r.uniform(-30, 30, shape)).astype(F) * np.where(r.random(shape) < 0.3, F(-1), F(1))
    out[wild] = mag[wild]
    tiny = sort == 3
    out[tiny] = (u * F(2.0 ** -66))[tiny]
    pick = r.random(shape)
    special = ~calm[:, None, None] & np.ones(shape, bool)
    out = np.where(special & (pick < 0.05), -out, out)
    out = np.where(special & (pick >= 0.05) & (pick < 0.08), F(0), out)
    out = np.where(special & (pick >= 0.08) & (pick < 0.10), F(-0.0), out)
    out = np.where(special & (pick >= 0.10) & (pick < 0.102), F(np.inf), out)
    out = np.where(special & (pick >= 0.102) & (pick < 0.104), F(-np.inf), out)
    if nan:
        out = np.where(r.random(shape) < 0.003, F(np.nan), out)
    out = np.ascontiguousarray(out, F)
    out.setflags(write=False)
    return out


def garbage(seed: int, shape) -> np.ndarray:
    """State a kernel must not read: large finite values, NaN and Inf."""
    r = np.random.default_rng(seed)
    g = (r.standard_normal(shape) * 1e30).astype(F)
    pick = r.random(shape)
    g = np.where(pick < 0.2, F(np.nan), g)
    return np.ascontiguousarray(np.where(pick > 0.9, F(np.inf), g), F)


# ---------------------------------------------------------------- window sums
def window(sample, acc, init, out=None, scale_ns=0):
    """launch_accumulate_window: returns (acc, out) with rows beyond the samples' untouched."""
    npix = sample.shape[0]
    acc = acc.copy()
    acc[:npix] = ordered_sum(np.zeros((npix, 3), F) if init else acc[:npix], sample)
    if out is not None:
        out = out.copy()
        with np.errstate(all="ignore"):
            out[:npix] = acc[:npix] * inv(scale_ns) if scale_ns else acc[:npix]
    return acc, out


# ---------------------------------------------------------------- adaptive folds
def new_state(n_slots: int, seed: int | None = None) -> dict:
    """sums [n, 3], mom [n, 2], mean [n, 3], count [n]: zeros, or (seeded) garbage with count 0."""
    if seed is None:
        return dict(sums=np.zeros((n_slots, 3), F), mom=np.zeros((n_slots, 2), F), mean=np.zeros((n_slots, 3), F),
                    count=np.zeros(n_slots, np.int32))
    return dict(sums=garbage(seed, (n_slots, 3)), mom=garbage(seed + 1, (n_slots, 2)), mean=garbage(seed + 2, (n_slots, 3)),
                count=np.zeros(n_slots, np.int32))


def copy_state(st: dict) -> dict:
    return {k: (None if v is None else v.copy()) for k, v in st.items()}


def _retired(count: np.ndarray, mom: np.ndarray, budget, min_spp, rel_tol, abs_eps) -> np.ndarray:
    return rr.retired(dict(count=count, s1=np.ascontiguousarray(mom[:, 0]), s2=np.ascontiguousarray(mom[:, 1])),
                      budget, min_spp, rel_tol, abs_eps)


def _fold_one(sums, mom, rgb, go):
    """One sample rgb[rows, 3] into the rows `go` of sums [rows, 3] and mom [rows, 2], in place."""
    with np.errstate(all="ignore"):
        y = ar.luminance(rgb[go])
        sums[go] = sums[go] + rgb[go]
        mom[go, 0] = mom[go, 0] + y
        mom[go, 1] = mom[go, 1] + y * y


def adaptive_fold(sample, st, keep, active_slot=None, init=0, decide=0, n_new=1, budget=1, rel_tol=0.0, abs_eps=0.0):
    """AdaptiveFold: returns (state, keep).  st["count"] may be None."""
    rows = sample.shape[0]
    slot = np.arange(rows) if active_slot is None else active_slot
    st, keep = copy_state(st), keep.copy()
    sums = np.zeros((rows, 3), F) if init else st["sums"][slot]
    mom = np.zeros((rows, 2), F) if init else st["mom"][slot]
    for k in range(sample.shape[1]):
        _fold_one(sums, mom, sample[:, k], np.ones(rows, bool))
    st["sums"][slot] = sums
    st["mom"][slot] = mom
    if decide:
        ret = _retired(np.full(rows, n_new, np.int32), mom, budget, 0, rel_tol, abs_eps)
        keep[:] = np.where(ret, 0, 1)
        with np.errstate(all="ignore"):
            st["mean"][slot[ret]] = sums[ret] * inv(n_new)
        if st["count"] is not None:
            st["count"][slot[ret]] = n_new
    return st, keep


def spec_window(sample, st, keep, ctr, active_slot=None, *, n, w, s0, batch_spp, min_spp, budget, rel_tol, abs_eps):
    """AdaptiveSpecFold, one window: returns (state, keep, ctr, facts).  `facts` counts what
    happened in the window, for the preconditions of the cases: rows left alone because their
    count is not the base (mismatch) or because they are retired at a base that is a boundary
    (at_base), stops strictly inside a 16-sample chunk (inside), at the pass's end off the
    batch grid (end_off_grid), by budget and by rule, and rows folded although the rule holds
    for them at a base that is no boundary (rule_at_plain_base)."""
    rows, spp_w = sample.shape[:2]
    assert s0 + spp_w <= w
    slot = np.arange(rows) if active_slot is None else active_slot
    st, keep, ctr = copy_state(st), keep.copy(), ctr.copy()
    c0, c_end = n + s0, n + w
    sums, mom = st["sums"][slot], st["mom"][slot]
    facts = dict(mismatch=0, at_base=0, inside=0, end_off_grid=0, budget=0, rule=0, rule_at_plain_base=0)
    before = np.zeros(rows, bool)
    if c0 == 0:  # a slot without samples starts from zero, whatever the state holds
        sums[:], mom[:] = 0, 0
    if s0 > 0:
        before = st["count"][slot] != c0
        facts["mismatch"] = int(before.sum())
        at_c0 = _retired(np.full(rows, c0, np.int32), mom, budget, min_spp, rel_tol, abs_eps) & ~before
        if s0 % batch_spp == 0:
            facts["at_base"] = int(at_c0.sum())
            before |= at_c0
        else:
            facts["rule_at_plain_base"] = int(at_c0.sum())
    going = ~before
    stop = np.zeros(rows, np.int32)
    for k in range(spp_w):
        _fold_one(sums, mom, sample[:, k], going)
        c = c0 + k + 1
        if (c - n) % batch_spp != 0 and c != c_end:
            continue
        ret = going & _retired(np.full(rows, c, np.int32), mom, budget, min_spp, rel_tol, abs_eps)
        stop[ret] = c
        going &= ~ret
        if ret.any():
            facts["budget" if c >= budget else "rule"] += int(ret.sum())
            if (k + 1) % CHUNK != 0 and k + 1 != spp_w:
                facts["inside"] += int(ret.sum())
            if c == c_end and (c - n) % batch_spp != 0:
                facts["end_off_grid"] += int(ret.sum())
    done = ~before
    stopped = done & (stop > 0)
    st["sums"][slot[done]] = sums[done]
    st["mom"][slot[done]] = mom[done]
    st["count"][slot[done]] = np.where(stopped, stop, c0 + spp_w)[done]
    keep[done] = np.where(stopped, 0, 1)[done]
    with np.errstate(all="ignore"):
        st["mean"][slot[stopped]] = sums[stopped] * inv_many(stop[stopped])[:, None]
    ctr[0] += int(before.sum()) * spp_w + int((c0 + spp_w - stop[stopped]).sum())
    ctr[1] += int((stopped & (stop < budget)).sum())
    facts["rows"] = rows
    facts["kept"] = int((keep[done] == 1).sum())
    facts["stops"] = int(stopped.sum())
    return st, keep, ctr, facts


def window_plan(w: int, width: int):
    """(s0, spp_w) of the windows of `width` samples that tile a pass of w (the last one narrower)."""
    return [(s0, min(width, w - s0)) for s0 in range(0, w, width)]


def spec_pass(sample, st, active_slot, width, run=spec_window, **rule):
    """A whole pass window by window: sample[rows, w, 3].  Returns (state, keep, ctr, [facts]).
    Each window starts from the state, keep and counters the one before it left."""
    rows, w = sample.shape[:2]
    keep = np.full(rows, 7, np.uint8)
    ctr = np.zeros(2, np.uint64)
    facts = []
    for s0, spp_w in window_plan(w, width):
        part = np.ascontiguousarray(sample[:, s0:s0 + spp_w])
        res = run(part, st, keep, ctr, active_slot, w=w, s0=s0, **rule)
        st, keep, ctr = res[:3]
        facts.append(res[3] if len(res) > 3 else None)
    return st, keep, ctr, facts


# ---------------------------------------------------------------- level, select, finish
def level_finish(count, mom, sums, budget, min_spp, rel_tol, abs_eps):
    """launch_adaptive_level_select, then launch_adaptive_finish: dict(live, keep, level,
    n_live, below, mean)."""
    m = np.where((count > 0)[:, None], mom, F(0)).astype(F)  # no samples: no moments, whatever the state holds
    live = ~_retired(count.copy(), m, budget, min_spp, rel_tol, abs_eps)
    level = int(count[live].min()) if live.any() else INT_MAX
    with np.errstate(all="ignore"):
        mean = np.where((count > 0)[:, None], sums * inv_many(np.maximum(count, 1))[:, None], F(0)).astype(F)
    return dict(live=live.astype(np.uint8), keep=(live & (count == level)).astype(np.uint8), level=level,
                n_live=int(live.sum()), below=int((count < budget).sum()), mean=mean)


# ---------------------------------------------------------------- compaction
def compact(keep, active_slot=None, pixels=None):
    """launch_adaptive_compact: (slot_out, pixel_out) of the kept rows, in ascending row."""
    rows = np.flatnonzero(keep != 0).astype(np.int32)
    slot = rows if active_slot is None else active_slot[rows]
    return slot.astype(np.int32), (slot if pixels is None else pixels[slot]).astype(np.int32)


# ---------------------------------------------------------------- AOV folds
def aov_fold(val, acc, init, finish, ns, p0, albedo=None, normal=None, depth=None):
    """AovFold: returns (acc, albedo, normal, depth); word 7 of acc is left alone."""
    np_ = val.shape[0]
    acc = acc.copy()
    acc[:, :7] = ordered_sum(np.zeros((np_, 7), F) if init else acc[:, :7], val[:, :, :7])
    albedo, normal, depth = (None if a is None else a.copy() for a in (albedo, normal, depth))
    if finish:
        with np.errstate(all="ignore"):
            m = acc * inv(ns)
        if albedo is not None:
            albedo[p0:p0 + np_] = m[:, 0:3]
        if depth is not None:
            depth[p0:p0 + np_] = m[:, 3]
        if normal is not None:
            normal[p0:p0 + np_] = m[:, 4:7]
    return acc, albedo, normal, depth


def aov_fold_emission(emit, acc, s0, ns, p0, count, emission):
    """AovEmissionFold: returns (acc, emission); word 3 of acc is left alone."""
    np_, spp_b = emit.shape[:2]
    acc, emission = acc.copy(), emission.copy()
    ni = np.full(np_, ns, np.int64) if count is None else np.clip(count[p0:p0 + np_].astype(np.int64), 1, ns)
    s = np.zeros((np_, 3), F) if s0 == 0 else acc[:, :3].copy()
    with np.errstate(all="ignore"):
        for k in range(spp_b):
            go = s0 + k < ni
            s[go] = s[go] + emit[go, k, :3]
    has = s0 < ni  # else: the pixel's samples ended in an earlier batch
    acc[has, :3] = s[has]
    last = has & (ni <= s0 + spp_b)
    with np.errstate(all="ignore"):
        emission[p0:p0 + np_][last] = s[last] * inv_many(ni[last])[:, None]
    return acc, emission


# ---------------------------------------------------------------- finish and scatter
def finish(acc, ns):
    with np.errstate(all="ignore"):
        return (acc * inv(ns)).astype(F)


def scatter(packed, index, image):
    image = image.copy()
    image[index] = packed
    return image


# ---------------------------------------------------------------- the speculative cases
# Window widths of every case: 12, 16 and 20 take the 16-byte loads, 6, 14 and 18 the scalar ones
# (a pass's last, narrower window may take the other route).
SPEC_WIDTHS = (12, 16, 20, 6, 14, 18)
SPEC_RULE = dict(batch_spp=4, min_spp=8, rel_tol=0.05, abs_eps=1e-3)


@functools.lru_cache(maxsize=None)
def spec_case(name: str) -> dict:
    """"fresh": 300 slots (a partial second block) without samples and with garbage in the
    state, one pass of 38 samples to the budget: the pass ends off the batch grid, where the
    budget stops whatever the rule has left, and none stops below 24 samples.  "resumed": 600 slots folded to 8 samples and
    decided there; the survivors (an injective map into the 600) get one pass of 22 samples
    from 8, far below the budget of 64: it ends at 30, off the grid, where only the rule
    stops.  Returns dict(sample, state, active_slot, rule): read-only."""
    if name == "fresh":
        n_slots, n, w, budget = 300, 0, 38, 38
        st = new_state(n_slots, seed=11)
        st["count"] = np.random.default_rng(12).integers(-5, 99, n_slots).astype(np.int32)  # not read at s0 = 0
        active = None
        sample = samples(13, n_slots, w)
    else:
        n_slots, n, w, budget = 600, 8, 22, 64
        every = samples(21, n_slots, n + w)
        st, keep = adaptive_fold(np.ascontiguousarray(every[:, :n]), new_state(n_slots, seed=22), np.zeros(n_slots, np.uint8), None, init=1, decide=1,
                                 n_new=n, budget=budget, rel_tol=SPEC_RULE["rel_tol"], abs_eps=SPEC_RULE["abs_eps"])
        st["count"][keep == 1] = n
        active = np.flatnonzero(keep).astype(np.int32)
        active = np.ascontiguousarray(active[np.random.default_rng(23).permutation(active.size)])
        sample = np.ascontiguousarray(every[active, n:])
        sample.setflags(write=False)
    for a in list(st.values()) + ([active] if active is not None else []):
        a.setflags(write=False)
    rule = dict(SPEC_RULE, n=n, budget=budget)
    if name == "fresh":
        rule["min_spp"] = 24  # nothing stops in a pass's first window, at any of the widths
    return dict(sample=sample, state=st, active_slot=active, rule=rule)


# ---------------------------------------------------------------- the ordering inputs
ORDER_SPP = 36        # two full chunks of 16 and a tail of 4
ORDER_MIN_SHARE = 0.5  # of the rows: the in-order sum differs in bits from both other orders


def order_shares(sample: np.ndarray):
    """Shares of the rows of sample[rows, spp, 3] whose in-order float32 sum (any channel)
    differs in bits from the sum in reversed order, and from the sum of the in-order sums of
    its chunks of 16."""
    rows = sample.shape[0]
    zero = np.zeros((rows, 3), F)
    fwd = ordered_sum(zero, sample)
    rev = ordered_sum(zero, sample[:, ::-1])
    parts = np.stack([ordered_sum(zero, sample[:, k:k + CHUNK]) for k in range(0, sample.shape[1], CHUNK)], axis=1)
    chunked = ordered_sum(zero, parts)

    def differs(a):
        ok = ~(np.isnan(fwd) | np.isnan(a))
        return float(((fwd.view(np.uint32) != a.view(np.uint32)) & ok).any(axis=1).mean())
    return differs(rev), differs(chunked)


# ---------------------------------------------------------------- the level, select, finish cases
LEVEL_RULE = dict(budget=16, min_spp=8, rel_tol=0.05, abs_eps=1e-3)
LEVEL_SLOTS = (1, 255, 256, 257, 1000)
LEVEL_CASES = ("retired", "one_level", "levels")


@functools.lru_cache(maxsize=None)
def level_case(name: str, n_slots: int) -> dict:
    """dict(count, mom, sums), read-only.  "retired": every slot at the budget or converged.
    "one_level": every slot live at 8 samples.  "levels": counts 0 (garbage moments), 4, 8, 12
    and the budget with the moments of real folds, some replaced by NaN and by moments of
    negative variance (s2 * n < s1 * s1)."""
    r = np.random.default_rng(1000 + n_slots)
    every = samples(31 + n_slots, n_slots, 16)
    if name == "retired":
        count = np.where(r.random(n_slots) < 0.5, 16, 8).astype(np.int32)
    elif name == "one_level":
        count = np.full(n_slots, 8, np.int32)
    else:
        count = r.choice(np.array([0, 4, 8, 12, 16], np.int32), size=n_slots).astype(np.int32)
    sums, mom = np.zeros((n_slots, 3), F), np.zeros((n_slots, 2), F)
    for k in range(16):
        _fold_one(sums, mom, every[:, k], count > k)
    if name == "retired":  # constant rows: no variance, the rule holds
        mom[:, 0] = F(8.0)
        mom[:, 1] = F(8.0)
    elif name == "one_level":  # s2 n far above s1^2: never converged
        mom[:, 0] = F(1.0)
        mom[:, 1] = F(100.0)
    else:
        pick = r.random(n_slots)
        mom[pick < 0.08] = F(np.nan)
        mom[(pick >= 0.08) & (pick < 0.16)] = np.array([10.0, 1.0], F)
        mom[count == 0] = garbage(5, (int((count == 0).sum()), 2))
        sums[count == 0] = garbage(6, (int((count == 0).sum()), 3))
    for a in (count, mom, sums):
        a.setflags(write=False)
    return dict(count=count, mom=mom, sums=sums)


# ---------------------------------------------------------------- the compaction cases
COMPACT_ROWS = (1, 64, 255, 256, 257, 65536, 65537, 131073)
COMPACT_KEEPS = ("zeros", "ones", "last", "third_chunk", "p01", "p50", "p99", "bytes")
SCAN_CHUNK = 256 * 256  # rows per chunk of the block scan: 256 block counts of 256 rows


def compact_keep(name: str, n: int):
    """The keep bytes of a compaction case, or None where the case needs more rows."""
    r = np.random.default_rng(n)
    keep = np.zeros(n, np.uint8)
    if name == "ones":
        keep[:] = 1
    elif name == "last":
        keep[-1] = 1
    elif name == "third_chunk":  # one survivor, in the first row of the third chunk, behind two chunks' carry
        if n <= 2 * SCAN_CHUNK:
            return None
        keep[:2 * SCAN_CHUNK] = r.random(2 * SCAN_CHUNK) < 0.5
        keep[2 * SCAN_CHUNK] = 1
    elif name in ("p01", "p50", "p99"):
        keep[:] = r.random(n) < {"p01": 0.01, "p50": 0.5, "p99": 0.99}[name]
    elif name == "bytes":  # any non-zero byte keeps
        keep[:] = r.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    return keep


# ---------------------------------------------------------------- the emission counts
def emission_counts(n_shard: int, ns: int, s0: int, spp_b: int) -> np.ndarray:
    """Per-pixel counts of every class the emission fold tells apart for the batch [s0, s0 + spp_b)
    of a frame of ns samples, dealt round-robin: 0 and negative (clamped to 1), 1, strictly inside the
    batch, s0 (ended before), s0 + spp_b, ns, above ns (clamped)."""
    classes = [0, -3, 1, s0 + 1 + (spp_b - 1) // 2, s0, s0 + spp_b, ns, ns + 5]
    return np.array([classes[i % len(classes)] for i in range(n_shard)], np.int32)
