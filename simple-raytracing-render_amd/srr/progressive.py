"""Progressive rendering with resume.

The reference renders a frame in one pass (Raytracing_n.cpp:815-879).  Here a
frame can be built up in chunks of samples -- each a render of the next sample
range [samples, samples + n) with SRR_FLAG_CONTINUE, added to the renderer's
per-pixel running sums in sample order -- and its state saved and resumed in
another process.  Per-path seeds and Sobol points depend only on (pixel, global
sample index), so any chunking gives bitwise the image of one render of all the
samples (tests/test_progressive.py).

With ``denoise`` set, step() returns the a-trous filtered frame (srr_denoise over
the first-hit AOVs, rendered once at ``aov_spp`` samples); the running sums and
``mean`` stay the undenoised ones, so the filter never feeds back into the frame.
``aov_through_specular`` takes the guides of either denoiser from the first hit that is
neither metal nor dielectric (srr_render_aov_through) instead of the first hit.

With ``adaptive`` set the frame is an adaptive one (srr_render_adaptive, continued by
srr_render_adaptive_resume): step(spp) raises the per-pixel budget by spp, pixels stop
on their own once they meet the tolerance, ``count`` holds each pixel's samples, and
the saved state is the adaptive state (sums, moments, counts).  A pixel that holds
n_i samples is bitwise the fixed-spp frame at n_i, however the budget was stepped.
``pass_spp_max`` / ``fill_paths`` switch the renderer's speculative passes on
(srr_adaptive_speculate): the same frames in fewer passes.
``denoise`` may then also be a capi.DenoiseVarParams: step() returns srr_denoise_var
of the mean, the variance of the pixels' mean luminance and the AOVs.
``denoise_emission`` filters the frame less its emission (srr_render_aov_emission over the
samples the frame holds -- per-pixel counts for an adaptive frame --, rendered again
whenever those change) and adds it back: srr_denoise_emission / srr_denoise_var_emission.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from . import capi


class Progressive:
    def __init__(self, renderer: "capi.Renderer", nx: int, ny: int, max_depth: int = 50, flags: int = 0,
                 denoise=None, aov_spp: int = 16, adaptive=None, pass_spp_max: int = 0, fill_paths: int = 0,
                 aov_through_specular: bool = False, denoise_emission: bool = False, **params):
        self.r = renderer
        self.nx, self.ny, self.max_depth = nx, ny, max_depth
        self.flags = flags  # engine flags (e.g. capi.FLAG_WAVEFRONT)
        self.params = params  # shard / tile / base_seed ... (capi.make_params keywords)
        self.samples = 0
        self.mean = None
        # adaptive: None / False (fixed spp per step), True (the defaults of
        # capi.Renderer.render_adaptive) or a capi.AdaptiveParams
        if adaptive is True:
            adaptive = capi.AdaptiveParams(ctypes.sizeof(capi.AdaptiveParams), 16, 16, 0.02, 1e-3)
        self.adaptive = adaptive or None
        # adaptive: speculative passes (capi.Renderer.adaptive_speculate) for every step; the frame does not change
        if pass_spp_max or fill_paths:
            if self.adaptive is None:
                raise capi.SrrError("pass_spp_max and fill_paths are an adaptive frame's: set adaptive")
            renderer.adaptive_speculate(pass_spp_max, fill_paths)
        self.count = None     # adaptive: samples per pixel
        self._resumable = False  # adaptive: the renderer holds this frame's state
        if isinstance(denoise, capi.DenoiseVarParams) and self.adaptive is None:
            raise capi.SrrError("a DenoiseVarParams needs the variance of an adaptive frame: set adaptive")
        # denoise: None / False (off), True (srr_denoise_defaults) or a capi.DenoiseParams
        self.denoise = capi.DenoiseParams.defaults() if denoise is True else (denoise or None)
        self.aov_spp = aov_spp
        self.aov_through_specular = bool(aov_through_specular)
        self.denoise_emission = bool(denoise_emission)
        if self.denoise_emission and self.denoise is None:
            raise capi.SrrError("denoise_emission needs a denoiser: set denoise")
        self.denoised = None
        self._aov = None
        if self.denoise is not None and params.get("shard", (0, 1))[1] > 1:
            raise capi.SrrError("a denoised progressive frame is the whole image: no shard")

    def step(self, spp: int) -> np.ndarray:
        """Render the next `spp` samples of every pixel; returns the mean over all
        samples so far (before the reference's sqrt / 8-bit tone map).  Adaptive:
        raise every pixel's budget by `spp` and render what the tolerance asks for."""
        if self.adaptive is not None:
            return self._step_adaptive(spp)
        flags = self.flags | (capi.FLAG_CONTINUE if self.samples else 0)
        out = self.r.render(self.nx, self.ny, spp, self.max_depth, sample_begin=self.samples, flags=flags,
                            **self.params)
        self.samples += spp
        self.mean = out["mean"]
        if self.denoise is None:
            return self.mean
        if self._aov is None:  # the AOV call leaves the running sums alone
            self._aov = self._render_aov()
        shape = (self.ny, self.nx, 3)
        a = self._aov
        self.denoised = capi.denoise(self.mean.reshape(shape), a["albedo"].reshape(shape), a["normal"].reshape(shape),
                                     a["depth"].reshape(self.ny, self.nx), self.denoise,
                                     emission=self._render_emission(self.samples, None)).reshape(-1, 3)
        return self.denoised

    def _render_aov(self) -> dict:
        kw = {k: v for k, v in self.params.items() if k in ("base_seed", "batch_paths")}
        return self.r.render_aov(self.nx, self.ny, self.aov_spp, max_depth=self.max_depth,
                                 through_specular=self.aov_through_specular, **kw)

    def _render_emission(self, spp: int, count):
        """The emission of the samples the frame holds now ([ny, nx, 3]), or None when not asked for."""
        if not self.denoise_emission:
            return None
        kw = {k: v for k, v in self.params.items() if k in ("base_seed", "batch_paths")}
        em = self.r.render_aov(self.nx, self.ny, spp, capi.AOV_EMISSION, max_depth=self.max_depth,
                               through_specular=self.aov_through_specular, count=count, **kw)["emission"]
        return em.reshape(self.ny, self.nx, 3)

    def _step_adaptive(self, spp: int) -> np.ndarray:
        a = self.adaptive
        render = self.r.render_adaptive_resume if self._resumable else self.r.render_adaptive
        out = render(self.nx, self.ny, self.samples + spp, self.max_depth, batch_spp=a.batch_spp, min_spp=a.min_spp,
                     rel_tol=a.rel_tol, abs_eps=a.abs_eps, flags=self.flags, **self.params)
        self._resumable = True
        self.samples += spp  # the budget so far
        self.mean, self.count, self.stats = out["mean"], out["count"], out["stats"]
        if self.denoise is None:
            return self.mean
        if self._aov is None:  # the AOV call leaves the adaptive state alone
            self._aov = self._render_aov()
        shape = (self.ny, self.nx, 3)
        aov = self._aov
        feats = (aov["albedo"].reshape(shape), aov["normal"].reshape(shape), aov["depth"].reshape(self.ny, self.nx))
        emission = self._render_emission(self.samples, self.count)  # (a pixel's count never exceeds the budget)
        if isinstance(self.denoise, capi.DenoiseVarParams):
            # (no shard: the shard's pixel order is PPM order, nothing to scatter)
            var = self.r.adaptive_variance(self.count).reshape(self.ny, self.nx)
            den, _ = capi.denoise_var(self.mean.reshape(shape), var, *feats, self.denoise, want_var=False,
                                      emission=emission)
        else:
            den = capi.denoise(self.mean.reshape(shape), *feats, self.denoise, emission=emission)
        self.denoised = den.reshape(-1, 3)
        return self.denoised

    def image8(self) -> np.ndarray:
        return capi.tonemap(self.mean)

    # ------------------------------------------------------------ resume
    def _scene_key(self) -> str:
        text = getattr(self.r.scene, "text", None)
        return hashlib.sha256(text.encode()).hexdigest() if isinstance(text, str) else ""

    def save(self, path: str) -> None:
        """Per-pixel running sums + sample count + frame parameters (.npz); adaptive:
        the adaptive state (sums, moments, counts), the budget so far and base_seed."""
        if self.adaptive is not None:
            st = self.r.adaptive_state()
            np.savez(path, sums=st["sums"], mom=st["mom"], count=st["count"], samples=self.samples, nx=self.nx,
                     ny=self.ny, max_depth=self.max_depth, scene=self._scene_key(), adaptive=1,
                     base_seed=int(self.params.get("base_seed", 0)))
            return
        L = capi.lib()
        npix, samples = ctypes.c_int64(), ctypes.c_int64()
        capi._check(L.srr_accum_get(self.r.h, None, ctypes.byref(npix), ctypes.byref(samples)))
        sums = np.zeros((npix.value, 3), np.float32)
        capi._check(L.srr_accum_get(self.r.h, capi._ptr(sums), None, None))
        np.savez(path, sums=sums, samples=samples.value, nx=self.nx, ny=self.ny, max_depth=self.max_depth,
                 scene=self._scene_key())

    def load(self, path: str) -> None:
        """Restore a saved state into this renderer (same scene and frame)."""
        z = np.load(path, allow_pickle=False)
        if (int(z["nx"]), int(z["ny"]), int(z["max_depth"])) != (self.nx, self.ny, self.max_depth):
            raise capi.SrrError("saved state is for a different frame")
        key = self._scene_key()
        if key and str(z["scene"]) and str(z["scene"]) != key:
            raise capi.SrrError("saved state is for a different scene")
        if ("adaptive" in z.files) != (self.adaptive is not None):
            raise capi.SrrError("saved state is an adaptive frame's" if "adaptive" in z.files else
                                "saved state is not an adaptive frame's")
        if self.adaptive is not None:
            if int(z["base_seed"]) != int(self.params.get("base_seed", 0)):
                raise capi.SrrError("saved state is for a different base_seed")
            kw = {k: v for k, v in self.params.items() if k in ("shard", "tile")}
            self.r.set_adaptive_state(self.nx, self.ny, z["sums"], z["mom"], z["count"], **kw)
            self.samples = int(z["samples"])
            self.count = np.ascontiguousarray(z["count"], np.int32)
            self._resumable = True
            return
        sums = np.ascontiguousarray(z["sums"], np.float32)
        capi._check(capi.lib().srr_accum_set(self.r.h, capi._ptr(sums), sums.shape[0], int(z["samples"])))
        self.samples = int(z["samples"])
