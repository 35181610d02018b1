"""ctypes binding of libsrr.so (include/srr_capi.h) -- the host-side mirror of
the reference's render driver (``renderthread``/``main``,
Raytracing_n.cpp:815-952) over the C-ABI.  The HIP path is the only path:
if libsrr.so is missing or no GPU is visible, calls fail loudly."""
from __future__ import annotations

import ctypes
import os

import numpy as np

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SRR_LIB") or os.path.join(PKG, "libsrr.so")  # SRR_LIB: A/B builds
_LIB = None

FLAG_SORT_MATERIALS = 1
FLAG_KEEP_PATHS = 2
FLAG_COUNT_VISITS = 4
FLAG_WAVEFRONT = 8
FLAG_CONTINUE = 16
FLAG_SUMS = 32
AOV_ALBEDO = 1
AOV_NORMAL = 2
AOV_DEPTH = 4
AOV_EMISSION = 8
DENOISE_DEMODULATE = 1


class SrrError(RuntimeError):
    pass


class Params(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("spp", ctypes.c_int), ("max_depth", ctypes.c_int),
                ("tile", ctypes.c_int), ("shard_index", ctypes.c_int), ("shard_count", ctypes.c_int),
                ("batch_paths", ctypes.c_int), ("base_seed", ctypes.c_uint64), ("flags", ctypes.c_int),
                ("sample_begin", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [("world_rays", ctypes.c_int64), ("paths", ctypes.c_int64), ("trace_launches", ctypes.c_int64),
                ("trace_ms", ctypes.c_double), ("shade_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("bounces", ctypes.c_int64), ("box_tests", ctypes.c_int64), ("tri_tests", ctypes.c_int64),
                ("stack_overflows", ctypes.c_int64), ("deep_traversals", ctypes.c_int64),
                ("mixture_capped", ctypes.c_int64), ("walks_suspended", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdaptiveParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("batch_spp", ctypes.c_int), ("min_spp", ctypes.c_int),
                ("rel_tol", ctypes.c_float), ("abs_eps", ctypes.c_float)]


class AdaptiveStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("passes", ctypes.c_int32), ("paths", ctypes.c_int64),
                ("world_rays", ctypes.c_int64), ("pixels_retired", ctypes.c_int64), ("total_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class AdaptiveSpecStats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("windows", ctypes.c_int32), ("paths_traced", ctypes.c_int64),
                ("paths_discarded", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class AovStats(ctypes.Structure):
    """srr_aov_stats of srr_render_aov_through."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("longest_chain", ctypes.c_int32), ("paths", ctypes.c_int64),
                ("world_rays", ctypes.c_int64), ("chained_paths", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class DenoiseParams(ctypes.Structure):
    """srr_denoise_params; ``DenoiseParams.defaults()`` is srr_denoise_defaults."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("iterations", ctypes.c_int), ("k_c", ctypes.c_float),
                ("k_n", ctypes.c_float), ("k_z", ctypes.c_float), ("flags", ctypes.c_int)]

    @classmethod
    def defaults(cls, **kw) -> "DenoiseParams":
        dp = cls()
        _check(lib().srr_denoise_defaults(ctypes.byref(dp)))
        for k, v in kw.items():
            setattr(dp, k, v)
        return dp


class DenoiseVarParams(ctypes.Structure):
    """srr_denoise_var_params; ``DenoiseVarParams.defaults()`` is srr_denoise_var_defaults."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("iterations", ctypes.c_int), ("k_l", ctypes.c_float),
                ("k_n", ctypes.c_float), ("k_z", ctypes.c_float), ("flags", ctypes.c_int)]

    @classmethod
    def defaults(cls, **kw) -> "DenoiseVarParams":
        dp = cls()
        _check(lib().srr_denoise_var_defaults(ctypes.byref(dp)))
        for k, v in kw.items():
            setattr(dp, k, v)
        return dp


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SrrError(f"{LIB_PATH} not built (run __graft_entry__.build() or make -C simple-raytracing-render_amd)")
        # One HIP runtime per process: torch ships its own libamdhip64.so.7 (the same SONAME
        # as /opt/rocm's, which libsrr.so's RUNPATH names), and whichever is loaded first
        # serves both.  Loaded first, /opt/rocm's left torch unable to initialise the GPU
        # afterwards ("No HIP GPUs are available", tools/torch_after_render.py), so when
        # torch is installed its runtime is loaded before libsrr.so.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, ip, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
        L.srr_last_error.restype = cp
        L.srr_version.restype = cp
        L.srr_scene_from_text.argtypes = [cp, ctypes.POINTER(vp)]
        L.srr_scene_destroy.argtypes = [vp]
        L.srr_renderer_create.argtypes = [vp, ip, ctypes.POINTER(vp)]
        L.srr_renderer_destroy.argtypes = [vp]
        L.srr_renderer_create_multi.argtypes = [vp, ip, vp, ctypes.POINTER(vp)]
        L.srr_renderer_devices.argtypes = [vp, vp, ip]
        L.srr_renderer_transport.argtypes = [vp]
        L.srr_renderer_transport.restype = cp
        L.srr_multi_plan.restype = ctypes.c_int64
        L.srr_multi_plan.argtypes = [ctypes.POINTER(Params), ip, vp, vp]
        L.srr_shard_pixels.restype = ctypes.c_int64
        L.srr_shard_pixels.argtypes = [ctypes.POINTER(Params), vp]
        L.srr_render_device.argtypes = [vp, ctypes.POINTER(Params), vp, ctypes.POINTER(Stats)]
        L.srr_render_device_async.argtypes = [vp, ctypes.POINTER(Params), vp, ctypes.POINTER(ctypes.c_int64)]
        L.srr_render_wait.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(Stats)]
        L.srr_merl_load.argtypes = [cp, ip, ctypes.POINTER(vp)]
        L.srr_merl_create.argtypes = [vp, ctypes.c_int64, ip, ctypes.POINTER(vp)]
        L.srr_merl_destroy.argtypes = [vp]
        L.srr_merl_lookup.argtypes = [vp, ctypes.c_int64, vp, vp, vp]
        L.srr_render.argtypes = [vp, ctypes.POINTER(Params), vp, vp, ctypes.POINTER(Stats)]
        L.srr_copy_paths.argtypes = [vp, vp, vp]
        L.srr_tonemap.argtypes = [vp, ctypes.c_int64, vp]
        L.srr_write_ppm.argtypes = [cp, ip, ip, vp]
        L.srr_sobol_points.argtypes = [ip, vp]
        L.srr_mesh_file_triangles.argtypes = [cp, ip, ip, vp, vp, vp, vp, ctypes.POINTER(ip)]
        u8p = ctypes.POINTER(ctypes.c_ubyte)
        L.srr_image_load.argtypes = [cp, ip, ctypes.POINTER(ip), ctypes.POINTER(ip), ctypes.POINTER(ip),
                                     ctypes.POINTER(u8p)]
        L.srr_image_free.argtypes = [u8p]
        L.srr_image_free.restype = None
        L.srr_write_png.argtypes = [cp, ip, ip, vp]
        i64p = ctypes.POINTER(ctypes.c_int64)
        L.srr_accum_get.argtypes = [vp, vp, i64p, i64p]
        L.srr_accum_set.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64]
        if hasattr(L, "srr_render_adaptive"):  # (an older A/B library under SRR_LIB lacks it: calls then fail by name)
            L.srr_render_adaptive.argtypes = [vp, ctypes.POINTER(Params), ctypes.POINTER(AdaptiveParams), vp, vp,
                                              ctypes.POINTER(AdaptiveStats)]
            L.srr_render_adaptive_host.argtypes = [vp, ctypes.POINTER(Params), ctypes.POINTER(AdaptiveParams), vp,
                                                   vp, vp, ctypes.POINTER(AdaptiveStats)]
            L.srr_adaptive_converged.argtypes = [ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                 ctypes.c_float]
        if hasattr(L, "srr_render_adaptive_resume"):  # (as above)
            L.srr_render_adaptive_resume.argtypes = L.srr_render_adaptive.argtypes
            L.srr_render_adaptive_resume_host.argtypes = L.srr_render_adaptive_host.argtypes
            L.srr_adaptive_state_get.argtypes = [vp, vp, vp, vp, i64p]
            L.srr_adaptive_state_set.argtypes = [vp, ctypes.POINTER(Params), vp, vp, vp, ctypes.c_int64]
        if hasattr(L, "srr_adaptive_speculate"):  # (as above)
            L.srr_adaptive_speculate.argtypes = [vp, ip, ctypes.c_int64]
            L.srr_adaptive_last_spec_stats.argtypes = [vp, ctypes.POINTER(AdaptiveSpecStats)]
            L.srr_adaptive_pass_width.argtypes = [ctypes.c_int64, ip, ip, ip, ip, ctypes.c_int64]
            L.srr_adaptive_fill_default.argtypes = []
            L.srr_adaptive_fill_default.restype = ctypes.c_int64
        if hasattr(L, "srr_denoise"):  # (as above)
            dpp = ctypes.POINTER(DenoiseParams)
            L.srr_render_aov.argtypes = [vp, ctypes.POINTER(Params), ip, vp, vp, vp]
            L.srr_render_aov_host.argtypes = [vp, ctypes.POINTER(Params), ip, vp, vp, vp]
            L.srr_denoise_defaults.argtypes = [dpp]
            L.srr_denoise.argtypes = [ip, ip, ip, dpp, vp, vp, vp, vp, vp]
            L.srr_denoise_host.argtypes = [ip, ip, ip, dpp, vp, vp, vp, vp, vp]
        if hasattr(L, "srr_render_aov_through"):  # (as above)
            L.srr_render_aov_through.argtypes = [vp, ctypes.POINTER(Params), ip, vp, vp, vp, ctypes.POINTER(AovStats)]
            L.srr_render_aov_through_host.argtypes = L.srr_render_aov_through.argtypes
        if hasattr(L, "srr_denoise_var"):  # (as above)
            dvp = ctypes.POINTER(DenoiseVarParams)
            L.srr_variance_of_mean.argtypes = [ctypes.c_int32, ctypes.c_float, ctypes.c_float]
            L.srr_variance_of_mean.restype = ctypes.c_float
            L.srr_adaptive_variance.argtypes = [vp, vp, vp]
            L.srr_adaptive_variance_host.argtypes = [vp, vp, vp]
            L.srr_denoise_var_defaults.argtypes = [dvp]
            L.srr_denoise_var.argtypes = [ip, ip, ip, dvp, vp, vp, vp, vp, vp, vp, vp]
            L.srr_denoise_var_host.argtypes = [ip, ip, ip, dvp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "srr_render_aov_emission"):  # (as above)
            L.srr_render_aov_emission.argtypes = [vp, ctypes.POINTER(Params), ip, ip, vp, vp, vp, vp, vp,
                                                  ctypes.POINTER(AovStats)]
            L.srr_render_aov_emission_host.argtypes = L.srr_render_aov_emission.argtypes
            L.srr_denoise_emission.argtypes = [ip, ip, ip, dpp, vp, vp, vp, vp, vp, vp]
            L.srr_denoise_emission_host.argtypes = L.srr_denoise_emission.argtypes
            L.srr_denoise_var_emission.argtypes = [ip, ip, ip, dvp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.srr_denoise_var_emission_host.argtypes = L.srr_denoise_var_emission.argtypes
        _LIB = L
    return _LIB


def _check(rc):
    if rc < 0:
        raise SrrError(f"srr error {rc}: {lib().srr_last_error().decode()}")
    return rc


def _ptr(a):
    return None if a is None else a.ctypes.data


def make_params(nx, ny, spp, max_depth=50, shard=(0, 1), tile=32, batch_paths=0, base_seed=0, flags=0,
                sample_begin=0):
    return Params(nx, ny, spp, max_depth, tile, shard[0], shard[1], batch_paths, base_seed, flags, sample_begin)


def shard_pixels(p: Params) -> np.ndarray:
    n = _check(lib().srr_shard_pixels(ctypes.byref(p), None))
    out = np.zeros(n, np.int32)
    lib().srr_shard_pixels(ctypes.byref(p), _ptr(out))
    return out


def multi_plan(p: Params, n_devices: int) -> tuple[np.ndarray, np.ndarray]:
    """srr_multi_plan (host only): the packed-frame order of an n-device frame --
    (gather_index[nx*ny]: image pixel of each packed entry, shard_offsets[n+1])."""
    total = _check(lib().srr_multi_plan(ctypes.byref(p), n_devices, None, None))
    index = np.zeros(total, np.int32)
    off = np.zeros(n_devices + 1, np.int64)
    _check(lib().srr_multi_plan(ctypes.byref(p), n_devices, _ptr(index), _ptr(off)))
    return index, off


def sobol_points(n: int) -> np.ndarray:
    out = np.zeros((n, 2), np.float64)
    _check(lib().srr_sobol_points(n, _ptr(out)))
    return out


class Scene:
    """A scene parsed from srr scene description v1 text."""

    def __init__(self, text: str):
        h = ctypes.c_void_p()
        _check(lib().srr_scene_from_text(text.encode(), ctypes.byref(h)))
        self.h = h
        self.text = text

    def __del__(self):
        if getattr(self, "h", None):
            lib().srr_scene_destroy(self.h)
            self.h = None


MERL_CELLS = 90 * 90 * 180  # doubles per channel of a MERL table (brdf.h:7-9)


class Merl:
    """A MERL measured-BRDF table on the GPU: the reference's ``brdf`` class
    (brdf.h).  ``Merl.load(path)`` is brdf::read_brdf, ``Merl(table)`` takes the
    3 * 90*90*180 doubles directly, ``lookup`` is brdf::lookup_brdf_val for a
    batch of (theta_in, fi_in, theta_out, fi_out) rows."""

    def __init__(self, table=None, device: int = 0, _handle=None):
        self.h = _handle
        if self.h is None:
            t = np.ascontiguousarray(table, dtype=np.float64).ravel()
            h = ctypes.c_void_p()
            _check(lib().srr_merl_create(t.ctypes.data, t.size, device, ctypes.byref(h)))
            self.h = h

    @classmethod
    def load(cls, path: str, device: int = 0) -> "Merl":
        h = ctypes.c_void_p()
        _check(lib().srr_merl_load(path.encode(), device, ctypes.byref(h)))
        return cls(_handle=h)

    def lookup(self, angles) -> tuple[np.ndarray, np.ndarray]:
        """angles: [n, 4] (theta_in, fi_in, theta_out, fi_out) -> (rgb [n, 3] f64, cell [n] int32)."""
        a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1, 4)
        rgb = np.zeros((a.shape[0], 3), np.float64)
        cell = np.zeros(a.shape[0], np.int32)
        _check(lib().srr_merl_lookup(self.h, a.shape[0], a.ctypes.data, rgb.ctypes.data, cell.ctypes.data))
        return rgb, cell

    def __del__(self):
        if getattr(self, "h", None) and _LIB is not None:
            _LIB.srr_merl_destroy(self.h)
            self.h = None


class Renderer:
    """Flattened scene resident on HIP device `device` (srr_renderer_create), or
    on every device of `devices` (srr_renderer_create_multi: the whole frame
    rendered over all of them, gathered to devices[0] over RCCL)."""

    def __init__(self, scene, device: int = 0, devices=None):
        if isinstance(scene, str):
            scene = Scene(scene)
        self.scene = scene
        h = ctypes.c_void_p()
        if devices is None:
            _check(lib().srr_renderer_create(scene.h, device, ctypes.byref(h)))
        else:
            ids = np.ascontiguousarray(devices, np.int32)
            _check(lib().srr_renderer_create_multi(scene.h, ids.size, _ptr(ids), ctypes.byref(h)))
        self.h = h

    def devices(self) -> list:
        n = _check(lib().srr_renderer_devices(self.h, None, 0))
        ids = np.zeros(n, np.int32)
        lib().srr_renderer_devices(self.h, _ptr(ids), n)
        return ids.tolist()

    @property
    def transport(self) -> str:
        """"rccl" / "copy" (multi-device frame-end gather) or "none" (one device)."""
        return lib().srr_renderer_transport(self.h).decode()

    def __del__(self):
        if getattr(self, "h", None):
            lib().srr_renderer_destroy(self.h)
            self.h = None

    def render(self, nx, ny, spp, max_depth=50, keep_paths=False, **kw):
        """Whole image (or shard); returns dict(mean[n,3], img8[n,3], stats,
        paths[n,spp,3], rays[n,spp] when keep_paths)."""
        flags = kw.pop("flags", 0) | (FLAG_KEEP_PATHS if keep_paths else 0)
        p = make_params(nx, ny, spp, max_depth, flags=flags, **kw)
        n = nx * ny if self.transport != "none" else shard_pixels(p).size
        mean = np.zeros((n, 3), np.float32)
        img8 = np.zeros((n, 3), np.uint8)
        st = Stats()
        _check(lib().srr_render(self.h, ctypes.byref(p), _ptr(mean), _ptr(img8), ctypes.byref(st)))
        out = dict(mean=mean, img8=img8, stats=st.as_dict())
        if keep_paths:
            paths = np.zeros((n, spp, 3), np.float32)
            rays = np.zeros((n, spp), np.uint8)
            _check(lib().srr_copy_paths(self.h, _ptr(paths), _ptr(rays)))
            out.update(paths=paths, rays=rays)
        return out

    def render_adaptive(self, nx, ny, max_spp, max_depth=50, batch_spp=16, min_spp=16, rel_tol=0.02, abs_eps=1e-3,
                        **kw):
        """Adaptive sampling (srr_render_adaptive): every pixel gets samples in
        passes of batch_spp until its luminance's relative standard error is at
        most rel_tol (not before min_spp samples) or it holds max_spp.  Returns
        dict(mean[n,3], count[n], img8[n,3], stats); kw: shard, tile, base_seed,
        flags, and struct_size (the srr_adaptive_params size the caller claims)."""
        size = kw.pop("struct_size", ctypes.sizeof(AdaptiveParams))
        p = make_params(nx, ny, max_spp, max_depth, **kw)
        a = AdaptiveParams(size, batch_spp, min_spp, rel_tol, abs_eps)
        n = nx * ny if self.transport != "none" else shard_pixels(p).size
        mean = np.zeros((n, 3), np.float32)
        count = np.zeros(n, np.int32)
        img8 = np.zeros((n, 3), np.uint8)
        st = AdaptiveStats(ctypes.sizeof(AdaptiveStats))
        _check(lib().srr_render_adaptive_host(self.h, ctypes.byref(p), ctypes.byref(a), _ptr(mean), _ptr(count),
                                              _ptr(img8), ctypes.byref(st)))
        return dict(mean=mean, count=count, img8=img8, stats=st.as_dict())

    def render_adaptive_device(self, params: Params, adaptive: AdaptiveParams, d_mean_ptr: int,
                               d_count_ptr: int = 0) -> dict:
        """srr_render_adaptive into device buffers (e.g. torch tensors' data_ptr())."""
        st = AdaptiveStats(ctypes.sizeof(AdaptiveStats))
        _check(lib().srr_render_adaptive(self.h, ctypes.byref(params), ctypes.byref(adaptive),
                                         ctypes.c_void_p(d_mean_ptr), ctypes.c_void_p(d_count_ptr or None),
                                         ctypes.byref(st)))
        return st.as_dict()

    def render_adaptive_resume(self, nx, ny, max_spp, max_depth=50, batch_spp=16, min_spp=16, rel_tol=0.02,
                               abs_eps=1e-3, **kw):
        """Continue the renderer's adaptive state (srr_render_adaptive_resume) under
        these parameters: arguments and result as render_adaptive; mean and count
        cover every pixel, stats this call's passes, paths and world rays."""
        size = kw.pop("struct_size", ctypes.sizeof(AdaptiveParams))
        p = make_params(nx, ny, max_spp, max_depth, **kw)
        a = AdaptiveParams(size, batch_spp, min_spp, rel_tol, abs_eps)
        n = nx * ny if self.transport != "none" else shard_pixels(p).size
        mean = np.zeros((n, 3), np.float32)
        count = np.zeros(n, np.int32)
        img8 = np.zeros((n, 3), np.uint8)
        st = AdaptiveStats(ctypes.sizeof(AdaptiveStats))
        _check(lib().srr_render_adaptive_resume_host(self.h, ctypes.byref(p), ctypes.byref(a), _ptr(mean),
                                                     _ptr(count), _ptr(img8), ctypes.byref(st)))
        return dict(mean=mean, count=count, img8=img8, stats=st.as_dict())

    def render_adaptive_resume_device(self, params: Params, adaptive: AdaptiveParams, d_mean_ptr: int,
                                      d_count_ptr: int = 0) -> dict:
        """srr_render_adaptive_resume into device buffers (e.g. torch tensors' data_ptr())."""
        st = AdaptiveStats(ctypes.sizeof(AdaptiveStats))
        _check(lib().srr_render_adaptive_resume(self.h, ctypes.byref(params), ctypes.byref(adaptive),
                                                ctypes.c_void_p(d_mean_ptr or None),
                                                ctypes.c_void_p(d_count_ptr or None), ctypes.byref(st)))
        return st.as_dict()

    def adaptive_speculate(self, pass_spp_max: int, fill_paths: int = 0) -> None:
        """Speculative passes (srr_adaptive_speculate) for the adaptive and resume calls
        that follow on this renderer: a pass may give a slot up to pass_spp_max samples,
        aiming at fill_paths paths (0: the library's default); pass_spp_max = 0 switches
        it off.  The frames' outputs do not change, only how many passes they take."""
        _check(lib().srr_adaptive_speculate(self.h, int(pass_spp_max), int(fill_paths)))

    def adaptive_spec_stats(self) -> dict:
        """dict(windows, paths_traced, paths_discarded) of the most recent adaptive or
        resume call on this renderer (srr_adaptive_last_spec_stats)."""
        st = AdaptiveSpecStats(ctypes.sizeof(AdaptiveSpecStats))
        _check(lib().srr_adaptive_last_spec_stats(self.h, ctypes.byref(st)))
        return st.as_dict()

    def adaptive_state(self) -> dict:
        """The adaptive state (srr_adaptive_state_get): dict(sums[n,3], mom[n,2] (s1, s2),
        count[n]) in shard-pixel order."""
        n = ctypes.c_int64()
        _check(lib().srr_adaptive_state_get(self.h, None, None, None, ctypes.byref(n)))
        out = dict(sums=np.zeros((n.value, 3), np.float32), mom=np.zeros((n.value, 2), np.float32),
                   count=np.zeros(n.value, np.int32))
        _check(lib().srr_adaptive_state_get(self.h, _ptr(out["sums"]), _ptr(out["mom"]), _ptr(out["count"]), None))
        return out

    def set_adaptive_state(self, nx, ny, sums, mom, count, npix=None, **kw) -> None:
        """Install an adaptive state (srr_adaptive_state_set) of the frame nx x ny (kw:
        shard, tile); npix defaults to count's size.  A render_adaptive_resume continues it."""
        p = make_params(nx, ny, 1, **kw)
        sums = np.ascontiguousarray(sums, np.float32)
        mom = np.ascontiguousarray(mom, np.float32)
        count = np.ascontiguousarray(count, np.int32).ravel()
        n = count.size if npix is None else int(npix)
        if sums.size != 3 * count.size or mom.size != 2 * count.size:
            raise SrrError("set_adaptive_state needs sums[n, 3], mom[n, 2] and count[n]")
        _check(lib().srr_adaptive_state_set(self.h, ctypes.byref(p), _ptr(sums), _ptr(mom), _ptr(count), n))

    def adaptive_variance(self, count) -> np.ndarray:
        """The variance of every pixel's mean luminance (srr_adaptive_variance_host) from
        the moments of the most recent successful render_adaptive on this renderer;
        count: that frame's counts.  Returns var[n] in shard-pixel order."""
        count = np.ascontiguousarray(count, np.int32).ravel()
        var = np.zeros(count.size, np.float32)
        _check(lib().srr_adaptive_variance_host(self.h, _ptr(count), _ptr(var)))
        return var

    def adaptive_variance_device(self, d_count_ptr: int, d_var_ptr: int) -> None:
        """srr_adaptive_variance over device buffers (e.g. torch tensors' data_ptr())."""
        _check(lib().srr_adaptive_variance(self.h, ctypes.c_void_p(d_count_ptr or None),
                                           ctypes.c_void_p(d_var_ptr or None)))

    def render_aov(self, nx, ny, spp, which=AOV_ALBEDO | AOV_NORMAL | AOV_DEPTH, max_depth=50,
                   through_specular=False, count=None, **kw):
        """First-hit feature buffers (srr_render_aov_host) of the samples
        [sample_begin, sample_begin + spp): dict(albedo[n,3], normal[n,3], depth[n])
        with the buffers selected in `which`; kw as make_params.  through_specular: the
        buffers of the first hit that is neither metal nor dielectric instead
        (srr_render_aov_through_host), and the call's srr_aov_stats under "stats".
        With AOV_EMISSION in `which` the call is srr_render_aov_emission_host: the dict
        gains emission[n,3] and "stats"; count[n] (int32, 1..spp) folds pixel i's emission
        over its first count[i] samples only."""
        p = make_params(nx, ny, spp, max_depth, **kw)
        n = shard_pixels(p).size
        out = {}
        if which & AOV_EMISSION:
            return self._render_aov_emission(p, n, which, through_specular, count)
        if count is not None:
            raise SrrError("render_aov: count= needs AOV_EMISSION in which")
        if which & AOV_ALBEDO:
            out["albedo"] = np.zeros((n, 3), np.float32)
        if which & AOV_NORMAL:
            out["normal"] = np.zeros((n, 3), np.float32)
        if which & AOV_DEPTH:
            out["depth"] = np.zeros(n, np.float32)
        bufs = (_ptr(out.get("albedo")), _ptr(out.get("normal")), _ptr(out.get("depth")))
        if through_specular:
            st = AovStats(ctypes.sizeof(AovStats))
            _check(lib().srr_render_aov_through_host(self.h, ctypes.byref(p), which, *bufs, ctypes.byref(st)))
            out["stats"] = st.as_dict()
        else:
            _check(lib().srr_render_aov_host(self.h, ctypes.byref(p), which, *bufs))
        return out

    def _render_aov_emission(self, p, n, which, through_specular, count):
        out = {}
        if which & AOV_ALBEDO:
            out["albedo"] = np.zeros((n, 3), np.float32)
        if which & AOV_NORMAL:
            out["normal"] = np.zeros((n, 3), np.float32)
        if which & AOV_DEPTH:
            out["depth"] = np.zeros(n, np.float32)
        out["emission"] = np.zeros((n, 3), np.float32)
        if count is not None:
            count = np.ascontiguousarray(count, np.int32).ravel()
            if count.size != n:
                raise SrrError("render_aov: count needs one int32 per shard pixel")
        st = AovStats(ctypes.sizeof(AovStats))
        _check(lib().srr_render_aov_emission_host(
            self.h, ctypes.byref(p), which, int(through_specular), _ptr(out.get("albedo")), _ptr(out.get("normal")), _ptr(out.get("depth")), _ptr(out["emission"]),
            _ptr(count), ctypes.byref(st)))
        out["stats"] = st.as_dict()
        return out

    def render_aov_device(self, params: Params, which: int, d_albedo_ptr: int = 0, d_normal_ptr: int = 0,
                          d_depth_ptr: int = 0, through_specular=False, d_emission_ptr: int = 0,
                          d_count_ptr: int = 0):
        """srr_render_aov into device buffers (e.g. torch tensors' data_ptr());
        through_specular: srr_render_aov_through, returning its stats as a dict.  With
        AOV_EMISSION in `which`: srr_render_aov_emission with d_emission_ptr and the optional
        d_count_ptr, returning its stats."""
        bufs = (ctypes.c_void_p(d_albedo_ptr or None), ctypes.c_void_p(d_normal_ptr or None),
                ctypes.c_void_p(d_depth_ptr or None))
        if which & AOV_EMISSION:
            st = AovStats(ctypes.sizeof(AovStats))
            _check(lib().srr_render_aov_emission(self.h, ctypes.byref(params), which, int(through_specular), *bufs,
                                                 ctypes.c_void_p(d_emission_ptr or None),
                                                 ctypes.c_void_p(d_count_ptr or None), ctypes.byref(st)))
            return st.as_dict()
        if not through_specular:
            _check(lib().srr_render_aov(self.h, ctypes.byref(params), which, *bufs))
            return None
        st = AovStats(ctypes.sizeof(AovStats))
        _check(lib().srr_render_aov_through(self.h, ctypes.byref(params), which, *bufs, ctypes.byref(st)))
        return st.as_dict()

    def render_device(self, params: Params, d_mean_ptr: int) -> dict:
        """Render into a device buffer (e.g. a torch tensor's data_ptr())."""
        st = Stats()
        _check(lib().srr_render_device(self.h, ctypes.byref(params), ctypes.c_void_p(d_mean_ptr), ctypes.byref(st)))
        return st.as_dict()

    def render_device_async(self, params: Params, d_mean_ptr: int) -> int:
        """Enqueue a fresh frame (srr_render_device_async); returns its ticket.
        d_mean is written when wait(ticket) returns."""
        t = ctypes.c_int64()
        _check(lib().srr_render_device_async(self.h, ctypes.byref(params), ctypes.c_void_p(d_mean_ptr),
                                             ctypes.byref(t)))
        return t.value

    def wait(self, ticket: int) -> dict:
        """Wait for an async frame (srr_render_wait); returns its stats."""
        st = Stats()
        _check(lib().srr_render_wait(self.h, ctypes.c_int64(ticket), ctypes.byref(st)))
        return st.as_dict()


def adaptive_pass_width(n_active, n, budget, batch_spp, pass_spp_max, fill_paths=0) -> int:
    """Samples per slot of the next speculative pass (srr_adaptive_pass_width; host, no GPU)."""
    return _check(lib().srr_adaptive_pass_width(int(n_active), int(n), int(budget), int(batch_spp),
                                                int(pass_spp_max), int(fill_paths)))


def adaptive_fill_default() -> int:
    """The fill_paths that 0 stands for (srr_adaptive_fill_default)."""
    return int(lib().srr_adaptive_fill_default())


def adaptive_converged(n, s1, s2, rel_tol, abs_eps) -> bool:
    """The convergence rule of srr_render_adaptive (srr_adaptive_converged; host, no GPU)."""
    return bool(lib().srr_adaptive_converged(int(n), float(s1), float(s2), float(rel_tol), float(abs_eps)))


def _emission_image(emission, color, fn):
    emission = np.ascontiguousarray(emission, np.float32)
    if emission.size != color.size:
        raise SrrError(f"{fn}: emission needs ny*nx*3 floats")
    return emission


def denoise(color, albedo, normal, depth, params: DenoiseParams = None, device: int = 0,
            emission=None) -> np.ndarray:
    """The a-trous denoiser (srr_denoise_host) over whole images in PPM order:
    color, albedo, normal [ny, nx, 3], depth [ny, nx] -> the filtered [ny, nx, 3].
    emission [ny, nx, 3]: filter color - emission and add it back (srr_denoise_emission_host)."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise SrrError("denoise needs color[ny, nx, 3]")
    ny, nx = color.shape[:2]
    albedo = np.ascontiguousarray(albedo, np.float32)
    normal = np.ascontiguousarray(normal, np.float32)
    depth = np.ascontiguousarray(depth, np.float32)
    if albedo.size != color.size or normal.size != color.size or depth.size * 3 != color.size:
        raise SrrError("denoise: albedo and normal need ny*nx*3 floats, depth ny*nx")
    dp = params if params is not None else DenoiseParams.defaults()
    out = np.zeros_like(color)
    if emission is not None:
        emission = _emission_image(emission, color, "denoise")
        _check(lib().srr_denoise_emission_host(device, nx, ny, ctypes.byref(dp), _ptr(color), _ptr(emission),
                                               _ptr(albedo), _ptr(normal), _ptr(depth), _ptr(out)))
        return out
    _check(lib().srr_denoise_host(device, nx, ny, ctypes.byref(dp), _ptr(color), _ptr(albedo), _ptr(normal),
                                  _ptr(depth), _ptr(out)))
    return out


def variance_of_mean(n, s1, s2) -> np.float32:
    """The variance of a pixel's mean luminance from its moments (srr_variance_of_mean; host, no GPU)."""
    return np.float32(lib().srr_variance_of_mean(int(n), float(s1), float(s2)))


def denoise_var(color, var, albedo, normal, depth, params: DenoiseVarParams = None, device: int = 0,
                want_var: bool = True, emission=None):
    """The variance-guided a-trous filter (srr_denoise_var_host) over whole images in PPM
    order: color, albedo, normal [ny, nx, 3], var, depth [ny, nx] -> (out [ny, nx, 3],
    var_out [ny, nx]); var_out is None when want_var is false (d_var_out = NULL).
    emission [ny, nx, 3]: filter color - emission and add it back (srr_denoise_var_emission_host)."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise SrrError("denoise_var needs color[ny, nx, 3]")
    ny, nx = color.shape[:2]
    var = np.ascontiguousarray(var, np.float32)
    albedo = np.ascontiguousarray(albedo, np.float32)
    normal = np.ascontiguousarray(normal, np.float32)
    depth = np.ascontiguousarray(depth, np.float32)
    if albedo.size != color.size or normal.size != color.size or depth.size * 3 != color.size or \
            var.size * 3 != color.size:
        raise SrrError("denoise_var: albedo and normal need ny*nx*3 floats, var and depth ny*nx")
    dp = params if params is not None else DenoiseVarParams.defaults()
    out = np.zeros_like(color)
    var_out = np.zeros((ny, nx), np.float32) if want_var else None
    if emission is not None:
        emission = _emission_image(emission, color, "denoise_var")
        _check(lib().srr_denoise_var_emission_host(device, nx, ny, ctypes.byref(dp), _ptr(color), _ptr(var),
                                                   _ptr(emission), _ptr(albedo), _ptr(normal), _ptr(depth),
                                                   _ptr(out), _ptr(var_out)))
        return out, var_out
    _check(lib().srr_denoise_var_host(device, nx, ny, ctypes.byref(dp), _ptr(color), _ptr(var), _ptr(albedo),
                                      _ptr(normal), _ptr(depth), _ptr(out), _ptr(var_out)))
    return out, var_out


def tonemap(mean: np.ndarray) -> np.ndarray:
    mean = np.ascontiguousarray(mean, np.float32)
    out = np.zeros(mean.shape, np.uint8)
    _check(lib().srr_tonemap(_ptr(mean), mean.size // 3, _ptr(out)))
    return out


def scene_digest(text: str) -> str:
    """srr_scene_digest of a scene description: the FNV-1a digest of its
    flattened device tables (hex), equal for byte-identical scenes."""
    L = lib()
    L.srr_scene_digest.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    h = ctypes.c_void_p()
    _check(L.srr_scene_from_text(text.encode(), ctypes.byref(h)))
    d = ctypes.c_uint64()
    try:
        _check(L.srr_scene_digest(h, ctypes.byref(d), None))
    finally:
        L.srr_scene_destroy(h)
    return f"{d.value:016x}"


MESH_KAT_VARIANTS = {"bvh2": 0, "bvh4": 1, "bvh4prune": 2, "quad": 3}


def device_mesh_kat(scene_text: str, rec: np.ndarray, variant: str, quad_max: int = 64, stack_cap: int = 8,
                    use_gstack: bool = True) -> np.ndarray:
    """srr_device_mesh_kat (test infrastructure): the `mesh` KAT's records with the
    outputs of the walker `variant` (MESH_KAT_VARIANTS) over scene_text's meshes."""
    L = lib()
    L.srr_device_mesh_kat.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    out = np.ascontiguousarray(rec, np.float32).copy()
    _check(L.srr_device_mesh_kat(scene_text.encode(), MESH_KAT_VARIANTS[variant], quad_max, stack_cap,
                                 1 if use_gstack else 0, out.shape[0], out.shape[1], _ptr(out)))
    return out


def device_world_kat(scene_text: str, rec: np.ndarray, tables: int) -> np.ndarray:
    """srr_device_world_kat (test infrastructure): the `world` KAT's records with the
    outputs of the world-list walk; tables 0 reads the world tables from global
    memory, 1 from their copy in LDS."""
    L = lib()
    L.srr_device_world_kat.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    out = np.ascontiguousarray(rec, np.float32).copy()
    _check(L.srr_device_world_kat(scene_text.encode(), tables, out.shape[0], out.shape[1], _ptr(out)))
    return out


def world_kat_counts(scene_text: str, world: int) -> dict:
    """srr_world_kat_counts (test infrastructure, no GPU): how a world of the `world`
    KAT's scene flattens."""
    L = lib()
    L.srr_world_kat_counts.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    c = np.zeros(5, np.int32)
    _check(L.srr_world_kat_counts(scene_text.encode(), world, _ptr(c)))
    return dict(objects=int(c[0]), sgroups=int(c[1]), obvhs=int(c[2]), leaves=int(c[3]), table_bytes=int(c[4]))


def device_bounce_kat(scene_text: str, rec: np.ndarray, variant: int, deep_tries: int = 32) -> np.ndarray:
    """srr_device_bounce_kat (test infrastructure): the `bounce` KAT's records with the
    outputs of one shading bounce; variant 0 the wavefront engine's scatter, 1 the path
    kernel's split diffuse bounce with its wave-cooperative mixture loop."""
    L = lib()
    L.srr_device_bounce_kat.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p]
    out = np.ascontiguousarray(rec, np.float32).copy()
    _check(L.srr_device_bounce_kat(scene_text.encode(), variant, deep_tries, out.shape[0], out.shape[1], _ptr(out)))
    return out


def bounce_kat_counts(scene_text: str, light_list: int) -> dict:
    """srr_bounce_kat_counts (test infrastructure, no GPU): how a light list of the
    `bounce` KAT's scene flattens."""
    L = lib()
    L.srr_bounce_kat_counts.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    c = np.zeros(6, np.int32)
    _check(L.srr_bounce_kat_counts(scene_text.encode(), light_list, _ptr(c)))
    return dict(lights=int(c[0]), none=int(c[1]), xz_rect=int(c[2]), sphere=int(c[3]), triangle=int(c[4]),
                materials=int(c[5]))


class FoldKat(ctypes.Structure):
    """srr_fold_kat of include/srr_capi.h."""
    _i, _p = ctypes.c_int32, ctypes.c_void_p
    _fields_ = [("sample", _p), ("rows", _i), ("spp", _i), ("misalign", _i), ("active_slot", _p), ("n_slots", _i),
                ("sums", _p), ("mom", _p), ("mean", _p), ("count", _p), ("count_out", _p), ("keep", _p), ("live", _p),
                ("lvl", _p), ("ctr", _p), ("init", _i), ("decide", _i), ("finish", _i), ("n", _i), ("w", _i),
                ("s0", _i), ("n_new", _i), ("batch_spp", _i), ("min_spp", _i), ("budget", _i), ("ns", _i),
                ("rel_tol", ctypes.c_float), ("abs_eps", ctypes.c_float), ("pixels", _p), ("index", _p),
                ("n_image", _i), ("slot_out", _p), ("pixel_out", _p), ("n_out", _p), ("p0", _i), ("n_shard", _i),
                ("albedo", _p), ("normal", _p), ("depth", _p), ("emission", _p), ("image", _p)]


# the arrays of FoldKat and their element types; a call checks dtype and contiguity, never converts
_FOLD_KAT_ARRAYS = dict(sample=np.float32, active_slot=np.int32, sums=np.float32, mom=np.float32, mean=np.float32,
                        count=np.int32, count_out=np.int32, keep=np.uint8, live=np.uint8, lvl=np.int32, ctr=np.uint64,
                        pixels=np.int32, index=np.int32, slot_out=np.int32, pixel_out=np.int32, n_out=np.int32,
                        albedo=np.float32, normal=np.float32, depth=np.float32, emission=np.float32, image=np.float32)


def device_fold_kat(kind: str, **fields) -> None:
    """srr_device_fold_kat (test infrastructure): one launch wrapper of the sample-folding
    and compaction kernels on host arrays.  Fields are those of srr_fold_kat; arrays are
    C-contiguous numpy arrays of the field's type, and the "io" ones are written in place.
    Array sizes are the caller's to get right (include/srr_capi.h gives them per kind)."""
    L = lib()
    L.srr_device_fold_kat.argtypes = [ctypes.c_char_p, ctypes.POINTER(FoldKat)]
    a = FoldKat()
    names = {f[0] for f in FoldKat._fields_}
    for k, v in fields.items():
        if k not in names:
            raise TypeError(f"srr_fold_kat has no field {k}")
        if k in _FOLD_KAT_ARRAYS:
            if v is None:
                continue
            if not (isinstance(v, np.ndarray) and v.dtype == _FOLD_KAT_ARRAYS[k] and v.flags.c_contiguous):
                raise TypeError(f"srr_fold_kat.{k}: a C-contiguous {np.dtype(_FOLD_KAT_ARRAYS[k]).name} array is required")
            setattr(a, k, v.ctypes.data)
        else:
            setattr(a, k, v)
    _check(L.srr_device_fold_kat(kind.encode(), ctypes.byref(a)))


def write_ppm(path: str, nx: int, ny: int, img8: np.ndarray) -> None:
    img8 = np.ascontiguousarray(img8, np.uint8)
    _check(lib().srr_write_ppm(path.encode(), nx, ny, _ptr(img8)))


def image_load(path: str, req_comp: int = 0) -> tuple[np.ndarray, int]:
    """stbi_load(path, &x, &y, &comp, req_comp) (stb_image v2.19, as the
    reference's builders call it): returns ``(pixels[y, x, channels], comp)``
    with comp the file's own channel count."""
    x, y, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    p = ctypes.POINTER(ctypes.c_ubyte)()
    ch = _check(lib().srr_image_load(path.encode(), req_comp, ctypes.byref(x), ctypes.byref(y), ctypes.byref(n),
                                     ctypes.byref(p)))
    try:
        px = np.ctypeslib.as_array(p, shape=(y.value, x.value, ch)).copy()
    finally:
        lib().srr_image_free(p)
    return px, n.value


def write_png(path: str, nx: int, ny: int, img8: np.ndarray) -> None:
    img8 = np.ascontiguousarray(img8, np.uint8)
    if img8.size != nx * ny * 3:
        raise SrrError("write_png needs nx*ny*3 bytes")
    _check(lib().srr_write_png(path.encode(), nx, ny, _ptr(img8)))


def mesh_file_triangles(path: str, flip_uvs: bool = False, flip_winding: bool = False, scale=(1.0, 1.0, 1.0)):
    """Mesh 0 of a PLY / binary FBX file as the reference's model loader builds it
    (model.h:28-59, geometry.h:24-79): returns ``(pos, uv, nrm, has_normals,
    has_uvs)`` with arrays of shape (n_tris, 3 corners, 3)."""
    sc = np.ascontiguousarray(scale, np.float32)
    fl = ctypes.c_int(0)
    n = _check(lib().srr_mesh_file_triangles(path.encode(), int(flip_uvs), int(flip_winding), _ptr(sc), None, None,
                                             None, ctypes.byref(fl)))
    pos, uv, nrm = (np.zeros((n, 3, 3), np.float32) for _ in range(3))
    _check(lib().srr_mesh_file_triangles(path.encode(), int(flip_uvs), int(flip_winding), _ptr(sc), _ptr(pos),
                                         _ptr(uv), _ptr(nrm), None))
    return pos, uv, nrm, bool(fl.value & 1), bool(fl.value & 2)
