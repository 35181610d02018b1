"""Device known-answer test of the kernels that turn samples into pixels
(k_accumulate_window, k_accumulate_window16, k_adaptive_fold, k_adaptive_fold_spec,
k_adaptive_level, k_adaptive_select, k_adaptive_finish, k_compact_count, k_compact_scan,
k_compact_scatter, k_aov_fold, k_aov_fold_emission, k_finish, k_scatter_pixels): each
launch wrapper of csrc/kernels.h runs on seeded synthetic buffers through
srr_device_fold_kat and is compared bit for bit with tests/fold_ref.py.  No tolerance
anywhere: floats by their bits (a NaN must be a NaN at the same place), integers by
equality, and every array a kernel must leave alone by the sentinel it went in with.
tests/test_fold_ref.py shows, without a GPU, that the cases hold what they are named for."""
import itertools

import numpy as np
import pytest

import fold_ref as fr
from srr import capi

pytestmark = pytest.mark.gpu

F = np.float32
ROWS = (1, 63, 64, 65, 255, 256, 257, 513)
WIDTHS = (1, 3, 4, 8, 12, 15, 16, 17, 20, 28, 32, 33, 36)
SENTINEL = F(-12345.5)


def filled(shape, value=SENTINEL, dtype=F):
    return np.full(shape, value, dtype)


def misaligns(spp):
    return (0, 1, 2, 3) if spp % 4 == 0 else (0,)  # only these widths choose their kernel by the pointer


# ---------------------------------------------------------------- window sums
OUT_MODES = (("absent", 0), ("raw", 0), ("mean", 1), ("mean", 3), ("mean", 344))


def device_window(sample, acc, init, out, scale_ns, misalign):
    acc = acc.copy()
    out = None if out is None else out.copy()
    capi.device_fold_kat("window", sample=sample, rows=sample.shape[0], spp=sample.shape[1], misalign=misalign,
                         n_slots=acc.shape[0], sums=acc, init=init, mean=out, ns=scale_ns)
    return acc, out


@pytest.mark.parametrize("rows", ROWS)
def test_window_sums(rows):
    """Every width, every misalignment that matters at it, and init and the output mode in turn
    (each pairing of them comes round over the widths); acc and out hold a sentinel past npix."""
    turn = itertools.cycle(itertools.product((1, 0), OUT_MODES))
    for spp in WIDTHS:
        sample = fr.samples(1000 * rows + spp, rows, spp, nan=True)
        for mis in misaligns(spp):
            init, (mode, ns) = next(turn)
            acc = filled((rows + 3, 3))
            acc[:rows] = fr.samples(5, rows, 1)[:, 0]
            out = None if mode == "absent" else filled((rows + 3, 3))
            want_acc, want_out = fr.window(sample, acc, init, out, ns)
            got_acc, got_out = device_window(sample, acc, init, out, ns, mis)
            what = f"rows {rows} spp {spp} misalign {mis} init {init} out {mode} {ns}"
            fr.same_bits(got_acc, want_acc, what + ": acc")
            if out is not None:
                fr.same_bits(got_out, want_out, what + ": out")


@pytest.mark.parametrize("rows", (255, 257, 513))
def test_window_sums_in_the_order_of_the_samples(rows):
    """The ordering inputs (tests/test_fold_ref.py: on most rows another order of the additions
    gives other bits) at a width with two full chunks and a tail, aligned and not."""
    sample = fr.samples(rows, rows, fr.ORDER_SPP, nan=True)
    acc = filled((rows, 3))
    want = fr.window(sample, acc, 1)[0]
    for mis in (0, 1, 2, 3):
        fr.same_bits(device_window(sample, acc, 1, None, 0, mis)[0], want, f"misalign {mis}")


@pytest.mark.parametrize("widths", ((16, 20), (12, 17, 36), (3, 32, 4)))
def test_window_sums_chained_through_acc(widths):
    rows = 257
    every = fr.samples(sum(widths), rows, sum(widths), nan=True)
    want_acc, want_out = fr.window(every, filled((rows, 3)), 1, filled((rows, 3)), 344)
    acc, out, s0 = filled((rows, 3)), None, 0
    for k, spp in enumerate(widths):
        last = k == len(widths) - 1
        acc, out = device_window(np.ascontiguousarray(every[:, s0:s0 + spp]), acc, 1 if k == 0 else 0,
                                 filled((rows, 3)) if last else None, 344, 0)
        s0 += spp
    fr.same_bits(acc, want_acc, "acc")
    fr.same_bits(out, want_out, "out")


# ---------------------------------------------------------------- adaptive fold
def device_adaptive_fold(sample, st, keep, active_slot, misalign=0, **f):
    st, keep = fr.copy_state(st), keep.copy()
    capi.device_fold_kat("adaptive_fold", sample=sample, rows=sample.shape[0], spp=sample.shape[1], misalign=misalign,
                         active_slot=active_slot, n_slots=st["sums"].shape[0], keep=keep, **st, **f)
    return st, keep


def same_state(got, want, what):
    for k in ("sums", "mom", "mean"):
        fr.same_bits(got[k], want[k], f"{what}: {k}")
    if want["count"] is not None:
        np.testing.assert_array_equal(got["count"], want["count"], err_msg=f"{what}: count")


def slot_map(seed, rows, n_slots):
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(n_slots)[:rows].astype(np.int32))


# init, decide, n_new against a budget of 16, rel_tol, a slot map, a count array
FOLD_MODES = ((1, 1, 8, 0.05, False, True), (0, 1, 8, 0.05, True, True), (0, 0, 8, 0.05, True, True),
              (1, 0, 8, 0.05, False, False), (0, 1, 16, 0.05, True, True), (0, 1, 20, 0.05, False, True),
              (0, 1, 8, 0.0, True, True), (1, 1, 8, 0.05, True, False))


@pytest.mark.parametrize("rows", ROWS)
def test_adaptive_fold(rows):
    """Widths on both sides of the 16-sample chunk and of the 16-byte loads, misaligned where
    that matters, with the modes in turn.  A state that is not started from zero holds real sums
    (and, past them, a sentinel that must survive in every slot the map does not name)."""
    turn = itertools.cycle(FOLD_MODES)
    decided = 0
    for spp in (1, 4, 15, 16, 17, 20, 36):
        sample = fr.samples(2000 * rows + spp, rows, spp)
        for mis in misaligns(spp):
            init, decide, n_new, rel_tol, mapped, counted = next(turn)
            n_slots = rows + 40 if mapped else rows + 2
            active = slot_map(rows + spp, rows, n_slots) if mapped else None
            st = dict(sums=filled((n_slots, 3)), mom=filled((n_slots, 2)), mean=filled((n_slots, 3)),
                      count=filled(n_slots, -77, np.int32) if counted else None)
            slot = np.arange(rows) if active is None else active
            prior = fr.adaptive_fold(fr.samples(3, rows, 4), fr.new_state(rows), np.zeros(rows, np.uint8), init=1)[0]
            st["sums"][slot], st["mom"][slot] = prior["sums"], prior["mom"]
            keep = filled(rows, 9, np.uint8)
            f = dict(init=init, decide=decide, n_new=n_new, budget=16, rel_tol=rel_tol, abs_eps=1e-3)
            want_st, want_keep = fr.adaptive_fold(sample, st, keep, active, **f)
            got_st, got_keep = device_adaptive_fold(sample, st, keep, active, mis, **f)
            what = f"rows {rows} spp {spp} misalign {mis} {f} mapped {mapped}"
            same_state(got_st, want_st, what)
            np.testing.assert_array_equal(got_keep, want_keep, err_msg=what)
            decided += int(decide and 0 < want_keep.sum() < rows)
    assert decided > 0 or rows < 63  # the rule decided both ways within a launch


# ---------------------------------------------------------------- speculative fold
def device_spec_window(sample, st, keep, ctr, active_slot, **f):
    st, keep, ctr = fr.copy_state(st), keep.copy(), ctr.copy()
    capi.device_fold_kat("adaptive_fold_spec", sample=sample, rows=sample.shape[0], spp=sample.shape[1],
                         active_slot=active_slot, n_slots=st["sums"].shape[0], keep=keep, ctr=ctr, **st, **f)
    return st, keep, ctr


@pytest.mark.parametrize("width", fr.SPEC_WIDTHS)
@pytest.mark.parametrize("name", ("fresh", "resumed"))
def test_speculative_fold_window_by_window(name, width):
    """A pass of fold_ref.spec_case window by window: after every window the device, which
    starts from the state its own previous window left, holds the restatement's state in
    every word of every slot, its keep bytes and both counters."""
    c = fr.spec_case(name)
    w = c["sample"].shape[1]
    st_d = st_r = c["state"]
    keep_d = keep_r = np.full(c["sample"].shape[0], 7, np.uint8)
    ctr_d = ctr_r = np.array([5, 1 << 33], np.uint64)  # the counters are added to
    for s0, spp_w in fr.window_plan(w, width):
        part = np.ascontiguousarray(c["sample"][:, s0:s0 + spp_w])
        st_r, keep_r, ctr_r, _ = fr.spec_window(part, st_r, keep_r, ctr_r, c["active_slot"], w=w, s0=s0, **c["rule"])
        st_d, keep_d, ctr_d = device_spec_window(part, st_d, keep_d, ctr_d, c["active_slot"], w=w, s0=s0, **c["rule"])
        what = f"{name} width {width} window at {s0}"
        same_state(st_d, st_r, what)
        np.testing.assert_array_equal(keep_d, keep_r, err_msg=what)
        np.testing.assert_array_equal(ctr_d, ctr_r, err_msg=what)


# ---------------------------------------------------------------- level, select, finish
@pytest.mark.parametrize("n_slots", fr.LEVEL_SLOTS)
@pytest.mark.parametrize("name", fr.LEVEL_CASES)
def test_level_select_finish(name, n_slots):
    c = fr.level_case(name, n_slots)
    want = fr.level_finish(**c, **fr.LEVEL_RULE)
    for with_count_out in (True, False):
        live, keep = filled(n_slots, 9, np.uint8), filled(n_slots, 9, np.uint8)
        lvl = np.array([-7, -8, -9, -10], np.int32)
        mean = filled((n_slots, 3))
        count_out = filled(n_slots, -77, np.int32) if with_count_out else None
        capi.device_fold_kat("level_finish", n_slots=n_slots, count=c["count"], mom=c["mom"], sums=c["sums"], live=live,
                             keep=keep, lvl=lvl, mean=mean, count_out=count_out, **fr.LEVEL_RULE)
        np.testing.assert_array_equal(live, want["live"])
        np.testing.assert_array_equal(keep, want["keep"])
        assert lvl.tolist() == [-7, want["level"], want["n_live"], want["below"]]
        fr.same_bits(mean, want["mean"], "mean")
        if with_count_out:
            np.testing.assert_array_equal(count_out, c["count"])


# ---------------------------------------------------------------- compaction
@pytest.mark.parametrize("rows", fr.COMPACT_ROWS)
def test_compaction(rows):
    for name, mapped in itertools.product(fr.COMPACT_KEEPS, (False, True)):
        keep = fr.compact_keep(name, rows)
        if keep is None:
            continue
        n_slots = rows + 100
        active = slot_map(rows, rows, n_slots) if mapped else None
        pixels = (np.random.default_rng(rows + 1).permutation(n_slots + 50)[:n_slots].astype(np.int32)) if mapped else None
        slot_out, pixel_out = filled(rows, -5, np.int32), filled(rows, -6, np.int32)
        n_out = np.array([-1], np.int32)
        capi.device_fold_kat("compact", rows=rows, keep=keep, active_slot=active, n_slots=n_slots, pixels=pixels,
                             n_image=n_slots + 50, slot_out=slot_out, pixel_out=pixel_out, n_out=n_out)
        want_slot, want_pixel = fr.compact(keep, active, pixels)
        what = f"rows {rows} keep {name} mapped {mapped}"
        assert int(n_out[0]) == want_slot.size, what
        np.testing.assert_array_equal(slot_out[:want_slot.size], want_slot, err_msg=what)
        np.testing.assert_array_equal(pixel_out[:want_slot.size], want_pixel, err_msg=what)
        assert (slot_out[want_slot.size:] == -5).all() and (pixel_out[want_slot.size:] == -6).all(), what


# ---------------------------------------------------------------- AOV folds
@pytest.mark.parametrize("spp_b", (1, 4, 7))
@pytest.mark.parametrize("np_", (1, 31, 32, 33, 257))
def test_aov_fold(np_, spp_b):
    """Two batches chained (init, then finish) at a pixel offset, each of the outputs absent in
    turn; word 7 of acc and the pixels outside [p0, p0 + np) keep their sentinel."""
    val = fr.samples(10 * np_ + spp_b, np_, 2 * spp_b, words=8, nan=True)
    p0, n_shard, ns = 5, np_ + 9, 2 * spp_b
    for absent in (None, "albedo", "normal", "depth"):
        outs = {k: (None if k == absent else filled((n_shard, 3) if k != "depth" else n_shard))
                for k in ("albedo", "normal", "depth")}
        acc_d = acc_r = filled((np_, 8))
        outs_d = outs_r = outs
        for b in (0, 1):
            part = np.ascontiguousarray(val[:, b * spp_b:(b + 1) * spp_b])
            f = dict(init=1 - b, finish=b, ns=ns, p0=p0)
            res = fr.aov_fold(part, acc_r, **f, **outs_r)
            acc_r, outs_r = res[0], dict(zip(("albedo", "normal", "depth"), res[1:]))
            acc_d = acc_d.copy()
            outs_d = {k: (None if v is None else v.copy()) for k, v in outs_d.items()}
            capi.device_fold_kat("aov_fold", sample=part, rows=np_, spp=spp_b, sums=acc_d, n_shard=n_shard, **f, **outs_d)
            fr.same_bits(acc_d, acc_r, f"acc, batch {b}, without {absent}")
            for k in outs:
                if outs[k] is not None:
                    fr.same_bits(outs_d[k], outs_r[k], f"{k}, batch {b}, without {absent}")
        assert (acc_d[:, 7] == SENTINEL).all()


@pytest.mark.parametrize("spp_b", (1, 4, 7))
@pytest.mark.parametrize("np_", (1, 31, 32, 33, 257))
@pytest.mark.parametrize("counted", (False, True))
def test_aov_fold_emission(counted, np_, spp_b):
    """Two batches chained, [0, spp_b) and [spp_b, 2 spp_b), of a frame of ns = 2 spp_b + 1 samples
    (so no pixel without a count gets its mean) and of ns = 2 spp_b; with counts, those of
    fold_ref.emission_counts for the second batch."""
    emit = fr.samples(20 * np_ + spp_b, np_, 2 * spp_b, words=4, nan=True)
    p0, n_shard = 3, np_ + 11
    for ns in (2 * spp_b, 2 * spp_b + 1):
        count = np.roll(fr.emission_counts(n_shard, ns, spp_b, spp_b), np_) if counted else None
        acc_d = acc_r = filled((np_, 4))
        em_d = em_r = filled((n_shard, 3))
        for b in (0, 1):
            part = np.ascontiguousarray(emit[:, b * spp_b:(b + 1) * spp_b])
            acc_r, em_r = fr.aov_fold_emission(part, acc_r, b * spp_b, ns, p0, count, em_r)
            acc_d, em_d = acc_d.copy(), em_d.copy()
            capi.device_fold_kat("aov_fold_emission", sample=part, rows=np_, spp=spp_b, s0=b * spp_b, sums=acc_d, ns=ns,
                                 p0=p0, n_shard=n_shard, count=count, emission=em_d)
            fr.same_bits(acc_d, acc_r, f"acc, batch {b}, ns {ns}")
            fr.same_bits(em_d, em_r, f"emission, batch {b}, ns {ns}")
        assert (acc_d[:, 3] == SENTINEL).all()


# ---------------------------------------------------------------- finish and scatter
@pytest.mark.parametrize("ns", (1, 3, 1024))
@pytest.mark.parametrize("n", (1, 255, 257))
def test_finish_and_scatter(n, ns):
    acc = np.ascontiguousarray(fr.samples(n + ns, n, 1, nan=True)[:, 0])
    mean = filled((n, 3))
    capi.device_fold_kat("finish", rows=n, sums=acc, ns=ns, mean=mean)
    fr.same_bits(mean, fr.finish(acc, ns), "mean")
    n_image = n + 30
    index = np.ascontiguousarray(np.random.default_rng(n).permutation(n_image)[:n].astype(np.int32))
    image = filled((n_image, 3))
    want = fr.scatter(acc, index, image)
    capi.device_fold_kat("scatter", sample=acc, rows=n, index=index, n_image=n_image, image=image)
    fr.same_bits(image, want, "image")
