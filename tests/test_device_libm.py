"""The libm restatements, function by function (csrc/glibc_mathf.h, include/srr/
glibc_math64.h), and the device libm behind the kernels' four double calls.

For every float routine the kernels call (devmath.h rsin ... ratan2, gm::sincosf_,
gm::atanf_) and every double routine restated from glibc (gm64 sin, cos, sincos,
acos, atan2 of the MERL lookup, log of the medium's hit distance), three results must be bit-identical on one shared input set
(tests/libm_inputs.py: every exponent and both signs, the subnormal range, the
specials, every branch edge of the routine +-64 ulps):

* the host's libm through oracle_libm (glibc 2.35 with the FMA ifunc variants,
  pinned by tests/golden/libm_pins.npz: on another libm the pins test fails and
  says so, instead of the comparisons below failing without a stated cause);
* the host build of the header (tests/cpp/libm_host.cpp, g++ -O2 -mfma
  -ffp-contract=off) -- CPU tests, with the one documented exception (expf, 1 ulp
  at 2 of the 2^32 inputs, listed by value);
* the device build (srr_device_libm) -- GPU tests, no exception.

The double calls that go to the device's own libm (sin / cos of both Beckmann
samplers, pow(., 5) of the dielectric) and the medium's log are checked at what
reaches a path: the float each call site stores, restated in
numpy from the raw double (exactly rounded steps only), against the same
expression on the host's double -- on sampled inputs and on the committed hard
cases (tests/golden/libm_hard.npz: every input whose call-site double lies within
64 ulps of a float rounding tie).  How often the raw doubles differ, and by how
many ulps at most, is printed, not asserted.  The medium's log was the device
libm's until this comparison found two of the 2^32 draws whose hit distance it
moved across a float rounding tie (density 0.0001 at k = 0xDABFD602, density 0.2 at
k = 0xEFF0E4B0, both in the hard set); it is gm64::log now, and the device libm's
log is still measured beside it.

numpy's own sin / log / exp are never the reference: they are not glibc."""
import ctypes
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import libm_inputs as li
import oracle_bind as ob
from srr import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32, F64 = np.float32, np.float64

RESTATED = sorted(li.FUNCS)

# expf_: the two inputs of the 2^32 where the restatement is 1 ulp off glibc's expf
# (glibc_mathf.h; found with tools/check_glibc_mathf.cpp's exhaustive sweep)
EXPF_EXCEPTIONS = np.array([0x4202422F, 0xC27C65D9], np.uint32)  # 0x1.04845ep+5, -0x1.f8cbb2p+5


# ---------------------------------------------------------------- the three builds

def host_libm(name, x, y):
    r = ob.libm(li.FUNCS[name][0], x, y)
    return r if isinstance(r, tuple) else (r,)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/cpp/libm_host.cpp built once per module, as tests/test_udiv.py and
    tests/test_merl.py build their helpers."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the host build of the headers"
    exe = tmp_path_factory.mktemp("libm_host") / "libm_host"
    subprocess.run([gxx, "-std=c++17", "-O2", "-mfma", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "libm_host.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def host_build(exe, name, x, y, tmp):
    """The header's host build on (x, y): a tuple of one or two result arrays."""
    _, dt, n_in, n_out = li.FUNCS[name]
    px, py, p0, p1 = (str(tmp / f"{name}.{s}") for s in ("x", "y", "o0", "o1"))
    x.tofile(px)
    if n_in == 2:
        y.tofile(py)
    subprocess.run([exe, name, px, py if n_in == 2 else "-", p0, p1 if n_out == 2 else "-"], check=True, timeout=120)
    out = tuple(np.fromfile(p, dtype=dt) for p in (p0, p1)[:n_out])
    for p in (px, py, p0, p1):
        if os.path.exists(p):
            os.remove(p)
    assert all(o.shape == x.shape for o in out)
    return out


def device_libm(name, x, y=None):
    """srr_device_libm on host arrays: a tuple of one or two result arrays."""
    L = capi.lib()
    L.srr_device_libm.restype = ctypes.c_int
    L.srr_device_libm.argtypes = [ctypes.c_char_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
    x = np.ascontiguousarray(x)
    y = None if y is None else np.ascontiguousarray(y, dtype=x.dtype)
    two = name in ("sincosf", "sincos64")
    o0 = np.empty_like(x)
    o1 = np.empty_like(x) if two else None
    capi._check(L.srr_device_libm(name.encode(), x.size, x.ctypes.data, None if y is None else y.ctypes.data,
                                  o0.ctypes.data, None if o1 is None else o1.ctypes.data))
    return (o0, o1) if two else (o0,)


def report(name, what, x, y, got, want, allowed=None):
    """Number of elements whose bits differ (two NaNs equal), the first few printed."""
    bad = np.zeros(x.shape, bool)
    for g, w in zip(got, want):
        bad |= ~li.same_bits(g, w)
    if allowed is not None:
        bad &= ~allowed
    idx = np.flatnonzero(bad)
    for i in idx[:6]:
        arg = f"x={float(x[i]).hex()}" + ("" if y is None else f" y={float(y[i]).hex()}")
        print(f"{name} {what}: {arg} got {[float(g[i]).hex() for g in got]} want {[float(w[i]).hex() for w in want]}")
    return len(idx)


# ---------------------------------------------------------------- CPU tests

def test_input_sets_hold_their_cases():
    """Every set has the subnormal range (smallest, largest, random), both signs,
    zeros, infinities, NaN, and its edges; the f64 sin / cos sets keep to the
    restatement's domain."""
    for name in RESTATED + ["rdiv"]:
        x, y = li.inputs(name)
        dt = x.dtype
        it = np.uint32 if dt == F32 else np.uint64
        tiny = np.finfo(dt).tiny
        for a in (x,) if y is None or name == "rpow" else (x, y):  # (powf's exponents are chosen by value)
            b = a.view(it)
            sub = (np.abs(a) < tiny) & (a != 0)
            assert sub.sum() >= 256 and (b == 1).any() and (b == (it(1) << it(23 if dt == F32 else 52)) - it(1)).any(), name
            assert (a == 0).any() and np.isinf(a).any() and np.isnan(a).any() and (a == 1).any() and (a == -1).any()
            assert (a == tiny).any() and np.signbit(a).any() and (~np.signbit(a)).any()
        n_exp = 256 if dt == F32 else 2048
        e = (np.abs(x).view(it) >> it(23 if dt == F32 else 52)).astype(np.int64)
        if name in ("sin64", "cos64", "sincos64"):
            fin = np.isfinite(x)
            assert (np.abs(x[fin]) < li.SIN64_LIMIT).all() and (np.abs(x[fin]) >= 1e8).any()
            assert set(range(0, 1023 + 27)) <= set(np.unique(e).tolist())
        else:
            assert np.unique(e).size == n_exp, name
    # +-64 ulps of an edge: 0.5 for acosf_, 88 for expf_, the double table rows
    for name, edge in (("racos", F32(0.5)), ("rexp", F32(88)), ("rsin", F32(120)), ("atanf", F32(0.4375))):
        x, _ = li.inputs(name)
        b = x.view(np.uint32).astype(np.int64)
        c = int(np.asarray(edge, F32).view(np.uint32))
        assert set(range(c - 64, c + 65)) <= set(b[(b >= c - 64) & (b <= c + 64)].tolist()), name
    x, y = li.inputs("rpow")
    with np.errstate(all="ignore"):
        r = ob.libm("powf", x, y)
    assert ((np.abs(r) < np.finfo(F32).tiny) & (r != 0)).sum() > 1000          # subnormal results
    assert ((r > F32(2.0 ** 126)) & np.isfinite(r)).sum() > 1000               # just below overflow
    a, b = li.inputs("rdiv")
    with np.errstate(all="ignore"):
        q = a / b
    assert ((np.abs(q) < np.finfo(F32).tiny) & (q != 0)).sum() > 100000
    qb = np.abs(q).view(np.uint32).astype(np.int64)
    assert ((qb >= 0x00800000 - 64) & (qb <= 0x00800000 + 64)).sum() > 10000


def test_oracle_libm_reproduces_the_pins():
    """oracle_libm on this machine is the libm the fixtures were recorded on (glibc
    2.35, FMA ifunc variants).  If this fails, the host's libm is another one: the
    host-build and device comparisons of this module would then fail for that
    reason alone, and tests/golden/make_libm_pins.py refuses to regenerate."""
    pins = np.load(os.path.join(GOLDEN, "libm_pins.npz"))
    names = sorted({k.split(".")[0] for k in pins.files if "." in k})
    assert names == sorted(ob.LIBM_F32 + ob.LIBM_F64)
    wrong = {}
    for name in names:
        x = pins[f"{name}.x"]
        y = pins[f"{name}.y"] if f"{name}.y" in pins.files else None
        assert x.size >= 2000
        got = ob.libm(name, x, y)
        got = got if isinstance(got, tuple) else (got,)
        want = tuple(pins[f"{name}.out{k}"] for k in range(len(got)))
        n = report(name, "oracle_libm against its pins", x, y, got, want)
        if n:
            wrong[name] = n
    assert not wrong, (f"this host's libm ({os.confstr('CS_GNU_LIBC_VERSION')}) does not reproduce the results "
                       f"recorded on {pins['libm'].item()}: {wrong}")


@pytest.mark.parametrize("name", RESTATED)
def test_host_build_matches_libm(name, host_exe, tmp_path):
    """The header's host build against the host's libm: what tools/check_glibc_mathf.cpp
    and tools/check_glibc_math64.cpp check, at the sweep's inputs."""
    x, y = li.inputs(name)
    if name == "rexp":
        x = np.concatenate([x, EXPF_EXCEPTIONS.view(F32)])
    want = host_libm(name, x, y)
    got = host_build(host_exe, name, x, y, tmp_path)
    allowed = None
    if name == "rexp":
        allowed = np.isin(x.view(np.uint32), EXPF_EXCEPTIONS)
        # the exception is real, and 1 ulp: if it goes away the list goes too
        d = got[0][allowed].view(np.uint32).astype(np.int64) - want[0][allowed].view(np.uint32).astype(np.int64)
        assert allowed.sum() >= 2 and (np.abs(d) == 1).all()
    n = report(name, "host build against libm", x, y, got, want, allowed)
    assert n == 0, f"{name}: {n} of {x.size} inputs differ between the header's host build and libm"


def test_unknown_names_are_refused():
    """Runs without a GPU: srr_device_libm checks every argument before its first HIP
    call (capi.cpp says so), and loading the library does not touch the device."""
    with pytest.raises(RuntimeError, match="no function named"):
        ob.libm("tanf", np.zeros(4, F32))
    x = np.zeros(4, F32)
    with pytest.raises(capi.SrrError):
        device_libm("tanf", x)
    with pytest.raises(capi.SrrError):
        device_libm("rpow", x)  # second operand missing
    L = capi.lib()
    assert L.srr_device_libm(b"rsin", 0, x.ctypes.data, None, x.ctypes.data, None) != 0
    assert L.srr_device_libm(b"rsin", 4, None, None, x.ctypes.data, None) != 0
    assert L.srr_device_libm(None, 4, x.ctypes.data, None, x.ctypes.data, None) != 0


# ---------------------------------------------------------------- GPU: the restatements

@pytest.mark.gpu
@pytest.mark.parametrize("name", RESTATED)
def test_device_build_matches_host_build(name, host_exe, tmp_path):
    """The device build of the header against its host build (which the CPU tests
    hold to libm): bit-identical on every input, no exception."""
    x, y = li.inputs(name)
    want = host_build(host_exe, name, x, y, tmp_path)
    t = time.perf_counter()
    got = device_libm(name, x, y)
    dt = time.perf_counter() - t
    n = report(name, "device build against host build", x, y, got, want)
    print(f"{name}: {x.size} inputs, {n} differ (device call {dt:.2f} s)")
    assert n == 0, f"{name}: {n} of {x.size} inputs differ between the device and the host build"


@pytest.mark.gpu
def test_device_division_is_correctly_rounded():
    """rdiv against numpy's float32 division (correctly rounded): subnormal
    quotients, quotients around FLT_MIN, every exponent pair class, specials."""
    a, b = li.inputs("rdiv")
    with np.errstate(all="ignore"):
        want = (a / b).astype(F32)
    got = device_libm("rdiv", a, b)
    n = report("rdiv", "device against numpy float32 division", a, b, got, (want,))
    assert n == 0, f"rdiv: {n} of {a.size} quotients differ"


# ---------------------------------------------------------------- the device libm's double calls

DENSITIES, INDICES, TWO_PI, pcg_u2 = li.DENSITIES, li.INDICES, li.TWO_PI, li.pcg_u2


def site_medium(density, log_u):
    """kernels.hip `float hit_distance = -(1 / md.density) * ::log(drand(rng));` (constant_medium.h:36):
    float( double(-(1.0f / density)) * log(u) )."""
    c = -(F32(1) / F32(density))
    with np.errstate(all="ignore"):
        return (F64(c) * log_u).astype(F32)


def site_beckmann(trig):
    """kernels.hip `float sinPhi = ::sin(2 * kPi * u2);` (microfacet_distribution.h:38-39): float( sin(.) )."""
    return trig.astype(F32)


def site_dielectric(ri, pow5):
    """kernels.hip `reflect_prob = r0 + (1 - r0) * ::pow((double)(1 - cosine), 5.0);` with float
    r0 = (1 - ri) / (1 + ri); r0 = r0 * r0 (material.h:14-19): float( double(r0) + double(1 - r0) * pow )."""
    ri = F32(ri)
    r0 = (F32(1) - ri) / (F32(1) + ri)
    r0 = F32(r0 * r0)
    return (F64(r0) + F64(F32(1) - r0) * pow5).astype(F32)


def sampled_u32():
    """All of [0, 2^16], the top 2^16, the powers of two +-8, 2^22 random (0 included: log 0)."""
    rng = np.random.default_rng([li.SEED, 32])
    p2 = (np.int64(1) << np.arange(0, 33, dtype=np.int64))[:, None] + np.arange(-8, 9, dtype=np.int64)[None, :]
    k = np.concatenate([np.arange(0, (1 << 16) + 1, dtype=np.int64), (1 << 32) - 1 - np.arange(1 << 16, dtype=np.int64),
                        p2.ravel(), rng.integers(0, 1 << 32, size=1 << 22, dtype=np.int64)])
    return np.unique(k[(k >= 0) & (k < (1 << 32))]).astype(np.uint32)


def sites(fn, x, dbl):
    """Every call-site float that the raw double results `dbl` of `fn` at x lead to."""
    if fn == "log":
        return {f"density {d}": site_medium(d, dbl) for d in DENSITIES}
    if fn == "pow":
        return {f"index {r}": site_dielectric(r, dbl) for r in INDICES}
    return {fn: site_beckmann(dbl)}


def ocml_inputs(fn, which):
    """(x of the double call, the host's doubles or None) of one function and input set."""
    if which == "hard":
        h = np.load(os.path.join(GOLDEN, "libm_hard.npz"))
        if fn == "log":
            return h["log.k"].astype(F64) / F64(4294967296.0), h["log.host"]
        return TWO_PI * h[f"{fn}.u2"].astype(F64), h[f"{fn}.host"]
    if fn == "log":
        return sampled_u32().astype(F64) / F64(4294967296.0), None
    if fn == "pow":
        rng = np.random.default_rng([li.SEED, 5])
        x = np.concatenate([rng.random(1 << 22, dtype=F32), F32([0, 1]), li.around([1.0, 0.5], F32)])
        return x[(x >= 0) & (x <= 1)].astype(F64), None
    return TWO_PI * np.unique(pcg_u2(sampled_u32())).astype(F64), None


OCML_CASES = [("log", "sampled"), ("log", "hard"), ("sin", "sampled"), ("sin", "hard"), ("cos", "sampled"),
              ("cos", "hard"), ("pow", "sampled")]


def host_double(fn, x):
    with np.errstate(all="ignore"):
        return ob.libm("pow", x, np.full_like(x, 5.0)) if fn == "pow" else ob.libm(fn, x)


@pytest.mark.parametrize("fn", ["log", "sin", "cos"])
def test_hard_cases_are_this_libm_and_hard(fn):
    """tests/golden/libm_hard.npz: the recorded host doubles are this host's libm, and
    every input is hard: for some call site its double lies within 64 ulps of a
    float rounding tie."""
    x, rec = ocml_inputs(fn, "hard")
    assert x.size > 0
    np.testing.assert_array_equal(host_double(fn, x).view(np.uint64), rec.view(np.uint64))
    near = np.zeros(x.shape, bool)
    for c in ([F64(-(F32(1) / F32(d))) for d in DENSITIES] if fn == "log" else [F64(1)]):
        low = ((c * rec).view(np.uint64) & np.uint64((1 << 29) - 1)).astype(np.int64)
        near |= np.abs(low - (1 << 28)) <= 64
    assert near.all()


def test_call_site_restatements_on_known_values():
    """The numpy restatements of the three call sites against hand-worked values."""
    assert site_medium(0.2, F64([-1.0]))[0] == F32(5.0) and site_medium(0.0001, F64([-0.5]))[0] == F32(5000.0)
    assert F32(-(F32(1) / F32(0.0001))) == F32(-10000.0)
    r0 = F32(F32(-0.5) / F32(2.5)) * F32(F32(-0.5) / F32(2.5))
    assert site_dielectric(1.5, F64([0.0, 1.0])).tolist() == [float(r0), 1.0]
    assert pcg_u2(np.uint32([0, 1, 0xFFFFFFFF, 0x80000000])).tolist() == [0.0, 2.0 ** -32, float(F32(0.99999994)), 0.5]


# what each call site runs on the device: the medium's log is the restatement, the others the device libm
DEVICE_FN = {"log": "log64", "sin": "ocml_sin", "cos": "ocml_cos", "pow": "ocml_pow5"}


def ulp_distance(a, b):
    """Largest distance in double ulps between two arrays, over the elements where both are finite."""
    fin = np.isfinite(a) & np.isfinite(b)
    def key(v):  # a monotonic integer key of a double
        u = v.view(np.int64)
        return np.where(u < 0, np.int64(-(1 << 63)) - u, u)
    d = np.abs(key(a[fin]) - key(b[fin]))
    return int(d.max()) if d.size else 0


@pytest.mark.gpu
@pytest.mark.parametrize("fn,which", OCML_CASES)
def test_device_double_calls_reach_the_paths_as_the_hosts(fn, which):
    """The float every call site stores is the same from the device's double as
    from the host's, on every input of the set, no exception."""
    x, rec = ocml_inputs(fn, which)
    host = host_double(fn, x) if rec is None else rec
    dev = device_libm(DEVICE_FN[fn], x)[0]
    raw = int((~li.same_bits(dev, host)).sum())
    print(f"device {DEVICE_FN[fn]} ({which}): {x.size} inputs, raw doubles differ on {raw} "
          f"({100.0 * raw / x.size:.4f} %), by at most {ulp_distance(dev, host)} ulps")
    if fn == "log":  # measured only: what the medium used before
        ocml = device_libm("ocml_log", x)[0]
        raw = int((~li.same_bits(ocml, host)).sum())
        moved = {s: int((~li.same_bits(v, sites(fn, x, ocml)[s])).sum()) for s, v in sites(fn, x, host).items()}
        print(f"device ocml_log ({which}): raw doubles differ on {raw} ({100.0 * raw / x.size:.4f} %), by at most "
              f"{ulp_distance(ocml, host)} ulps; call-site floats moved: {moved}")
    hs, ds = sites(fn, x, host), sites(fn, x, dev)
    wrong = {}
    for site in hs:
        bad = np.flatnonzero(~li.same_bits(hs[site], ds[site]))
        for i in bad[:6]:
            print(f"  {site}: x={float(x[i]).hex()} host {float(host[i]).hex()} -> {float(hs[site][i]).hex()}, "
                  f"device {float(dev[i]).hex()} -> {float(ds[site][i]).hex()}")
        if bad.size:
            wrong[site] = int(bad.size)
    assert not wrong, f"{fn} ({which}): call-site floats differ from the host's: {wrong} of {x.size}"
