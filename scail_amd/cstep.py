"""Binding of the C-level step executor (include/scail_dit.h, csrc/dit_step.hip): the whole network evaluation of one
sampler step is ONE call into libscail_hip.so -- the host only hands over device pointers.  Used by
``DiffusionTransformer`` when ``use_c_step`` is set (single sequence-parallel rank); the Python orchestration in
``dit._run`` stays as the multi-rank / instrumented path and as the cross-check (both enqueue the same kernels in the same
order, so their results are bit-identical)."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import lib as L

_p, _i64 = C.c_void_p, C.c_int64


class DitConfig(C.Structure):
    _fields_ = [("hidden_size", C.c_int32), ("num_heads", C.c_int32), ("inner_hidden_size", C.c_int32),
                ("num_layers", C.c_int32), ("text_dim", C.c_int32), ("clip_dim", C.c_int32),
                ("time_freq_dim", C.c_int32), ("time_embed_dim", C.c_int32), ("layernorm_epsilon", C.c_float)]


_LAYER_FIELDS = ["qkv_w", "qkv_b", "o_w", "o_b", "qn", "kn", "cq_w", "cq_b", "co_w", "co_b", "cqn", "ln_w", "ln_b",
                 "w1", "b1", "w2", "b2"]


class DitLayer(C.Structure):
    _fields_ = [(n, _p) for n in _LAYER_FIELDS]


class DitWeights(C.Structure):
    _fields_ = [(n, _p) for n in ("patch_w", "patch_b", "pose_w", "pose_b", "time0_w", "time0_b", "time2_w", "time2_b",
                                  "adaln_w", "adaln_b", "adaln_tables", "final_table", "final_w", "final_b")] + \
               [("layers", C.POINTER(DitLayer))]


class DitCond(C.Structure):
    _fields_ = [("k_text", _p), ("vt_text", _p), ("k_clip", _p), ("vt_clip", _p), ("Lt", _i64), ("Lc", _i64), ("Bc", _i64)]


# include/scail_dit.h "sequence-parallel execution": the exchange callback and its descriptor
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p)
SP_ALLGATHER, SP_ULYSSES = 0, 1
SP_FWD_START, SP_FWD_WAIT, SP_BACK_START, SP_BACK_WAIT = 0, 1, 2, 3


class DitSp(C.Structure):
    _fields_ = [("ranks", C.c_int32), ("mode", C.c_int32), ("send", _p), ("recv", _p), ("ofull", _p), ("back", _p),
                ("exchange", EXCHANGE_FN), ("user", _p), ("side_stream", _p * 2)]


def _cond_struct(cond: Dict) -> "DitCond":
    k_text, k_clip = cond["k_text"], cond["k_clip"]
    return DitCond(k_text.data_ptr(), cond["vt_text"].data_ptr(), k_clip.data_ptr(), cond["vt_clip"].data_ptr(),
                   k_text.shape[2], k_clip.shape[2], k_clip.shape[1])


class CStep:
    """Handle around scail_dit_create / scail_dit_step for one prepared network (``net.prepare()`` dict)."""

    def __init__(self, net, W: Dict):
        L.load()
        self._keep = W                                   # the pointer tables reference these tensors
        cfg = DitConfig(net.hidden_size, net.num_attention_heads, net.inner_hidden_size, net.num_layers, net.text_dim,
                        1280, net.time_freq_dim, net.time_embed_dim, float(net.layernorm_epsilon))
        layers = (DitLayer * net.num_layers)()
        for i, lw in enumerate(W["layers"]):
            for n in _LAYER_FIELDS:
                setattr(layers[i], n, lw[n].data_ptr())
        w = DitWeights(W["patch_w"].data_ptr(), W["patch_b"].data_ptr(), W["pose_w"].data_ptr(), W["pose_b"].data_ptr(),
                       W["time_embed.0.w"].data_ptr(), W["time_embed.0.b"].data_ptr(),
                       W["time_embed.2.w"].data_ptr(), W["time_embed.2.b"].data_ptr(),
                       W["adaln_projection.1.w"].data_ptr(), W["adaln_projection.1.b"].data_ptr(),
                       W["adaln_tables"].data_ptr(), W["final_table"].data_ptr(), W["final_w"].data_ptr(),
                       W["final_b"].data_ptr(), layers)
        h = _p()
        L.call("scail_dit_create", C.byref(cfg), C.byref(w), C.byref(h))
        self._h = h
        self._ws = None
        self._cache = None                               # ((B, T, H, W, device), buffer) of the step cache, once a FILL has run
        self._tile_cache = None                          # ((n_tiles, Tt, H, W, device), buffer) of the tiled sampler's cache (sample_tiled_cached)
        self._delta = None                               # ((T, H, W, device), buffer) of the guidance plan's delta (sample_guided)
        self._hist = None                                # ((T, H, W, device), buffer) of the solver plan's history (sample / sample_tiled)
        self._fp8_buf = None
        self._probe = None                               # (table, scratch) while the fp8 probe is on
        self.num_layers = net.num_layers
        self.fp8_scaling = getattr(net, "fp8_scaling", "row")   # lib.FP8_SCALINGS key that enable_fp8 uses when none is given
        if getattr(net, "fp8_mask", 0):
            if getattr(net, "gemm_precision", "fp8") == "fp6":
                self.enable_fp6(net.fp8_mask, W["patch_w"].device)
            else:
                self.enable_fp8(net.fp8_mask, W["patch_w"].device)
            if getattr(net, "fp8_layer_masks", None) is not None:
                self.select_fp8_layers(net.fp8_layer_masks)

    def enable_fp8(self, which: int, device, scaling=None) -> None:
        """scail_dit_enable_fp8_scaled: quantize the selected per-token GEMM weights (lib.FP8_GEMMS bits) into a buffer this object owns,
        under ``scaling`` ("row" | "mx", lib.FP8_SCALINGS; None: the network's); which = 0 returns to bf16."""
        lib = L.load()
        scaling = self.fp8_scaling if scaling is None else scaling
        if scaling not in L.FP8_SCALINGS:
            raise L.ScailHipError(f"enable_fp8: scaling must be one of {sorted(L.FP8_SCALINGS)}, got {scaling!r}")
        sc = L.FP8_SCALINGS[scaling]
        self._probe = None                               # the executor turns the probe off and forgets the per-layer selection
        if not which:
            L.call("scail_dit_enable_fp8", self._h, 0, None, 0, torch.cuda.current_stream(device).cuda_stream)
            self._fp8_buf = None
            return
        nbytes = lib.scail_dit_fp8_weight_bytes_scaled(self._h, which, sc)
        if nbytes < 0:
            raise L.ScailHipError(f"scail_dit_fp8_weight_bytes_scaled: bad mask {which}")
        buf = torch.empty(nbytes, device=device, dtype=torch.uint8)
        L.call("scail_dit_enable_fp8_scaled", self._h, which, sc, buf.data_ptr(), nbytes, torch.cuda.current_stream(device).cuda_stream)
        self._fp8_buf = buf
        self.fp8_scaling = scaling

    def enable_fp6(self, which: int, device) -> None:
        """scail_dit_enable_fp6: quantize the selected per-token GEMM weights (lib.FP8_GEMMS bits) to packed MXFP6 e2m3 into a buffer this
        object owns, replacing an fp8 form; which = 0 returns to bf16."""
        lib = L.load()
        self._probe = None                               # the executor turns the probe off and forgets the per-layer selection
        stream = torch.cuda.current_stream(device).cuda_stream
        if not which:
            L.call("scail_dit_enable_fp6", self._h, 0, None, 0, stream)
            self._fp8_buf = None
            return
        nbytes = lib.scail_dit_fp6_weight_bytes(self._h, which)
        if nbytes < 0:
            raise L.ScailHipError(f"scail_dit_fp6_weight_bytes: bad mask {which}")
        buf = torch.empty(nbytes, device=device, dtype=torch.uint8)
        L.call("scail_dit_enable_fp6", self._h, which, buf.data_ptr(), nbytes, stream)
        self._fp8_buf = buf

    def select_fp8_layers(self, masks) -> None:
        """scail_dit_fp8_select_layers: ``masks`` = one lib.FP8_GEMMS mask per layer, each a subset of the enabled mask (the GEMMs that
        stay fp8 in that layer); None = the enabled mask in every layer again."""
        if masks is None:
            L.call("scail_dit_fp8_select_layers", self._h, None)
            return
        masks = [int(m) for m in masks]
        if len(masks) != self.num_layers:
            raise L.ScailHipError(f"select_fp8_layers: need one mask per layer ({self.num_layers}), got {len(masks)}")
        if any(m < 0 or m > 0xffffffff for m in masks):
            raise L.ScailHipError(f"select_fp8_layers: masks must be unsigned 32-bit values, got {masks}")
        L.call("scail_dit_fp8_select_layers", self._h, (C.c_uint32 * len(masks))(*masks))

    def fp8_probe_on(self, B: int, Ltok: int, device) -> torch.Tensor:
        """scail_dit_fp8_probe: calls of up to B * Ltok token rows now also measure every quantised GEMM against its bf16 twin (and run
        the network in bf16).  Returns the zeroed device table (layers, 6, 4) fp64 the executor accumulates into."""
        need = L.load().scail_dit_fp8_probe_bytes(self._h, B, Ltok)
        if need < 0:
            raise L.ScailHipError(f"scail_dit_fp8_probe_bytes: bad shape (B {B}, Ltok {Ltok})")
        table = torch.zeros(self.num_layers, 6, 4, device=device, dtype=torch.float64)
        scratch = torch.empty(max(need, 256), device=device, dtype=torch.uint8)
        L.call("scail_dit_fp8_probe", self._h, table.data_ptr(), scratch.data_ptr(), scratch.numel())
        self._probe = (table, scratch)
        return table

    def fp8_probe_off(self) -> None:
        """Back to the selected kernels (the table the caller holds stays valid; the scratch is released in stream order)."""
        L.call("scail_dit_fp8_probe", self._h, None, None, 0)
        self._probe = None

    def close(self):
        if self._h is not None:
            L.load().scail_dit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    PROF_SELF_ATTN, PROF_GEMM, PROF_CROSS_ATTN = 0, 1, 2          # include/scail_dit.h SCAIL_DIT_PROF_*
    PROF_XCH_FWD_WAIT, PROF_XCH_BACK_WAIT = 3, 4                  # exposed part of the sequence-parallel exchange (stream waits)
    PROF_ATTN_RESTARTS = 5                                        # not a time: restarted self-attention workgroups (second value of profile_read)

    def profile(self, enable: bool) -> None:
        """HIP-event timing of the executor's own launches (scail_dit_profile): on = restart the counters."""
        L.call("scail_dit_profile", self._h, 1 if enable else 0)

    def profile_read(self, category: int):
        """(summed kernel ms, launches) of one category since profile(True); waits for the recorded events."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.call("scail_dit_profile_read", self._h, category, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def _ws_for(self, need: int, device, what: str) -> torch.Tensor:
        """The workspace, grown to ``need`` bytes on ``device``; ``what`` names the query that answered ``need`` and what it was asked."""
        if need < 0:
            raise L.ScailHipError(f"{what}: the executor has no workspace for this request (bad shape / mode)")
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, device=device, dtype=torch.uint8)
        return self._ws

    @staticmethod
    def _schedule(sigmas, device):
        """(timesteps (n, 2) device fp32 = 1000 sigma_i twice, sigma_{i+1} - sigma_i as a host float array, n) of the host schedule"""
        sig = sigmas.float().cpu()
        n = sig.numel() - 1
        ts = (sig[:-1] * 1000.0).repeat_interleave(2).to(device).contiguous()
        return ts, (C.c_float * n)(*[float(v) for v in (sig[1:] - sig[:-1])]), n

    def workspace_bytes(self, B, T, H, W, n_char: int = 1) -> int:
        n = L.load().scail_dit_chars_workspace_bytes(self._h, B, T, H, W, n_char)
        if n < 0:
            raise L.ScailHipError(f"scail_dit_chars_workspace_bytes: bad shape (B {B}, T {T}, H {H}, W {W}, n_char {n_char})")
        return n

    CFG_PAIR = 1                                                  # include/scail_dit.h SCAIL_DIT_CFG_PAIR

    def step(self, x32, t32, cond: Dict, ref, pose, cos, sin, cfg_pair: bool = False, n_char: int = 1) -> torch.Tensor:
        """``cfg_pair``: the caller states that x32 / t32 hold the same latent and timestep twice (VanillaCFG's batch of 2): layer 0 up to
        its first cross attention is evaluated once (SCAIL_DIT_CFG_PAIR; bit-identical on such inputs).  ``n_char``: characters in
        ``ref`` (n, n_char, 16, H, W) / ``pose`` (n, n_char * T, 16, H/2, W/2); cos / sin from rope.build_tables(n_char=n_char)."""
        B, T, _, H, W = x32.shape
        ws = self._ws_for(self.workspace_bytes(B, T, H, W, n_char), x32.device, "scail_dit_chars_workspace_bytes")
        cc = _cond_struct(cond)
        out = torch.empty(B, T, 16, H, W, device=x32.device, dtype=torch.float32)
        L.call("scail_dit_step_chars", self._h, x32.data_ptr(), t32.data_ptr(), C.byref(cc), ref.data_ptr(), ref.shape[0],
               pose.data_ptr(), pose.shape[0], n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), out.data_ptr(), B, T, H, W,
               self.CFG_PAIR if cfg_pair else 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return out

    # ---- solver plan (include/scail_dit.h "solver plan") ----
    def solver_bytes(self, T, H, W) -> int:
        n = L.load().scail_dit_solver_bytes(T, H, W)
        if n < 0:
            raise L.ScailHipError(f"scail_dit_solver_bytes: bad shape (T {T}, H {H}, W {W})")
        return n

    def _hist_for(self, T, H, W, device) -> torch.Tensor:
        """The history buffer of a (T, H, W) latent, a new one when the shape or the device changed.  Handed out by ``_ws_for`` and kept
        beside the workspace, as ``_cache_for`` does."""
        key = (T, H, W, torch.device(device))
        if self._hist is None or self._hist[0] != key:
            ws, self._ws = self._ws, None
            try:
                buf = self._ws_for(self.solver_bytes(T, H, W), device, f"scail_dit_solver_bytes (T {T}, H {H}, W {W})")
            finally:
                self._ws = ws
            self._hist = (key, buf)
        return self._hist[1]

    def solver_history(self, T, H, W) -> torch.Tensor:
        """The data prediction D (1, T, 16, H, W) fp32 of the last step of a solver loop: a view of the history buffer"""
        assert self._hist is not None and self._hist[0][:3] == (T, H, W), "no history buffer of this shape"
        return self._hist[1][:4 * T * 16 * H * W].view(torch.float32).view(1, T, 16, H, W)

    @staticmethod
    def solver_tables(solver, n):
        """The host arrays of a ``solver`` = (sigma, coef) option: (sigma fp32 [n], coef fp32 [n][3]); sigma = the steps' starting sigmas,
        coef = one (a, b, c) per step (sampler.plan_solver)."""
        sigma, coef = solver
        sg = [float(v) for v in (sigma.tolist() if torch.is_tensor(sigma) else sigma)]
        rows = [tuple(float(v) for v in r) for r in coef]
        if len(sg) != n or len(rows) != n or any(len(r) != 3 for r in rows):
            raise L.ScailHipError(f"solver: needs one starting sigma and one (a, b, c) per step ({n}), got {len(sg)} sigmas and {len(rows)} rows")
        return (C.c_float * max(n, 1))(*sg), (C.c_float * max(3 * n, 1))(*[v for r in rows for v in r])

    def sample(self, x32, sigmas, cfg_scale, cond: Dict, ref, pose, cos, sin, n_char: int = 1, solver=None) -> torch.Tensor:
        """The whole Euler loop in one C call (scail_dit_sample_chars).  x32 (1,T,16,H,W) fp32 is updated in place and returned;
        ``sigmas`` is the host schedule (n_steps + 1 values); ``cond`` the batch-2 conditioning (uncond, cond); ``n_char`` as for step.
        ``solver``: None, or (sigma, coef) -- the steps' starting sigmas and one (a, b, c) per step (sampler.plan_solver): the loop under a
        solver plan (scail_dit_sample_solver), still ONE call that only enqueues."""
        _, T, _, H, W = x32.shape
        if solver is not None:
            ts, dsa, n = self._schedule(sigmas, x32.device)
            sg, co = self.solver_tables(solver, n)
            hist = self._hist_for(T, H, W, x32.device)
            ws = self._ws_for(L.load().scail_dit_sample_chars_workspace_bytes(self._h, T, H, W, n_char), x32.device,
                              f"scail_dit_sample_chars_workspace_bytes (T {T}, H {H}, W {W}, n_char {n_char})")
            cc = _cond_struct(cond)
            assert x32.is_contiguous() and x32.dtype == torch.float32 and ref.shape[0] == 1 and pose.shape[0] == 1
            L.call("scail_dit_sample_solver", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale),
                   C.byref(cc), ref.data_ptr(), pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, W,
                   ws.data_ptr(), ws.numel(), sg, co, hist.data_ptr(), hist.numel(), torch.cuda.current_stream().cuda_stream)
            return x32
        ws = self._ws_for(L.load().scail_dit_sample_chars_workspace_bytes(self._h, T, H, W, n_char), x32.device,
                          f"scail_dit_sample_chars_workspace_bytes (T {T}, H {H}, W {W}, n_char {n_char})")
        ts, dsa, n = self._schedule(sigmas, x32.device)
        cc = _cond_struct(cond)
        assert x32.is_contiguous() and x32.dtype == torch.float32 and ref.shape[0] == 1 and pose.shape[0] == 1
        L.call("scail_dit_sample_chars", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale),
               C.byref(cc), ref.data_ptr(), pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, W,
               ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return x32

    # ---- step cache (include/scail_dit.h "step cache") ----
    def step_cache_bytes(self, B, T, H, W) -> int:
        n = L.load().scail_dit_step_cache_bytes(self._h, B, T, H, W)
        if n < 0:
            raise L.ScailHipError(f"scail_dit_step_cache_bytes: bad shape (B {B}, T {T}, H {H}, W {W})")
        return n

    def _cache_for(self, B, T, H, W, device, fill: bool) -> torch.Tensor:
        """The cache of a (B, T, H, W) evaluation.  A FILL gets a new one when the shape or the device changed; a REUSE needs the one a
        FILL of that shape left.  Handed out by ``_ws_for`` like every other buffer the executor is given, but kept beside the
        workspace: ``_ws_for`` is asked with no workspace in hand and the workspace is put back afterwards."""
        key = (B, T, H, W, torch.device(device))
        if self._cache is None or self._cache[0] != key:
            if not fill:
                raise L.ScailHipError(f"step cache: a 'reuse' evaluation of (B {B}, T {T}, H {H}, W {W}) needs a 'fill' evaluation of that shape first")
            ws, self._ws = self._ws, None
            try:
                buf = self._ws_for(self.step_cache_bytes(B, T, H, W), device, f"scail_dit_step_cache_bytes (B {B}, T {T}, H {H}, W {W})")
            finally:
                self._ws = ws
            self._cache = (key, buf)
        return self._cache[1]

    def step_cache_residual(self, B, T, H, W, D) -> torch.Tensor:
        """r (B, Lnoise, D) bf16 as the last FILL of this shape left it: a view of offset 0 of the cache"""
        assert self._cache is not None and self._cache[0][:4] == (B, T, H, W), "no cache of this shape"
        n = B * T * (H // 2) * (W // 2) * D
        return self._cache[1][:2 * n].view(torch.bfloat16).view(B, -1, D)

    def step_cached(self, x32, t32, cond, ref, pose, cos, sin, mode: str, cfg_pair: bool = False, n_char: int = 1, cache=None) -> torch.Tensor:
        """``step`` in a cache mode (scail_dit_step_cached): "fill" = the full evaluation, which also leaves the blocks' residual on the
        noise rows in the cache; "reuse" = patch embedding of the noise rows + that residual + the final layer (``cond`` may be None).
        ``cache``: None = the cache this object keeps (``_cache_for``), or a caller-owned uint8 tensor of at least ``step_cache_bytes`` on
        the latent's device, 256-byte aligned, which this object neither keeps nor checks against an earlier "fill"."""
        if mode not in L.CACHE_MODES:
            raise L.ScailHipError(f"step_cached: mode must be one of {sorted(L.CACHE_MODES)}, got {mode!r}")
        B, T, _, H, W = x32.shape
        if cache is None:
            cache = self._cache_for(B, T, H, W, x32.device, mode == "fill")
        elif cache.dtype != torch.uint8 or cache.dim() != 1 or not cache.is_contiguous() or cache.device != x32.device:
            raise L.ScailHipError(f"step_cached: a caller-owned cache is a contiguous 1-d uint8 tensor on {x32.device}, got {cache.dtype} "
                                  f"{tuple(cache.shape)} on {cache.device}")
        ws = self._ws_for(self.workspace_bytes(B, T, H, W, n_char), x32.device, "scail_dit_chars_workspace_bytes")
        cc = None if cond is None else _cond_struct(cond)
        out = torch.empty(B, T, 16, H, W, device=x32.device, dtype=torch.float32)
        L.call("scail_dit_step_cached", self._h, x32.data_ptr(), t32.data_ptr(), None if cc is None else C.byref(cc), ref.data_ptr(), ref.shape[0],
               pose.data_ptr(), pose.shape[0], n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), out.data_ptr(), B, T, H, W,
               self.CFG_PAIR if cfg_pair else 0, ws.data_ptr(), ws.numel(), L.CACHE_MODES[mode], cache.data_ptr(), cache.numel(),
               torch.cuda.current_stream().cuda_stream)
        return out

    def sample_cached(self, x32, sigmas, cfg_scale, cond: Dict, ref, pose, cos, sin, reuse, n_char: int = 1) -> torch.Tensor:
        """``sample`` with a step cache (scail_dit_sample_cached): ``reuse`` = one 0 / 1 per step (sampler.plan_step_cache), 1 = that step
        reuses the residual of the last computed step.  Still ONE call that only enqueues."""
        _, T, _, H, W = x32.shape
        ts, dsa, n = self._schedule(sigmas, x32.device)
        reuse = [int(v) for v in reuse]
        if len(reuse) != n:
            raise L.ScailHipError(f"sample_cached: the reuse mask needs one entry per step ({n}), got {len(reuse)}")
        if any(v < 0 or v > 255 for v in reuse):
            raise L.ScailHipError(f"sample_cached: the reuse mask holds 0 / 1 entries, got {reuse}")
        cache = self._cache_for(2, T, H, W, x32.device, True)
        ws = self._ws_for(L.load().scail_dit_sample_chars_workspace_bytes(self._h, T, H, W, n_char), x32.device,
                          f"scail_dit_sample_chars_workspace_bytes (T {T}, H {H}, W {W}, n_char {n_char})")
        cc = _cond_struct(cond)
        assert x32.is_contiguous() and x32.dtype == torch.float32 and ref.shape[0] == 1 and pose.shape[0] == 1
        L.call("scail_dit_sample_cached", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale),
               C.byref(cc), ref.data_ptr(), pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, W,
               ws.data_ptr(), ws.numel(), (C.c_uint8 * max(n, 1))(*reuse), cache.data_ptr(), cache.numel(), torch.cuda.current_stream().cuda_stream)
        return x32

    # ---- guidance plan (include/scail_dit.h "guidance plan") ----
    def guidance_bytes(self, T, H, W) -> int:
        n = L.load().scail_dit_guidance_bytes(T, H, W)
        if n < 0:
            raise L.ScailHipError(f"scail_dit_guidance_bytes: bad shape (T {T}, H {H}, W {W})")
        return n

    def _delta_for(self, T, H, W, device) -> torch.Tensor:
        """The delta buffer of a (T, H, W) latent, a new one when the shape or the device changed.  Handed out by ``_ws_for`` and kept beside
        the workspace, as ``_cache_for`` does."""
        key = (T, H, W, torch.device(device))
        if self._delta is None or self._delta[0] != key:
            ws, self._ws = self._ws, None
            try:
                buf = self._ws_for(self.guidance_bytes(T, H, W), device, f"scail_dit_guidance_bytes (T {T}, H {H}, W {W})")
            finally:
                self._ws = ws
            self._delta = (key, buf)
        return self._delta[1]

    def guidance_delta(self, T, H, W) -> torch.Tensor:
        """v_c - v_u (1, T, 16, H, W) fp32 as the last PAIR step of sample_guided left it: a view of the delta buffer"""
        assert self._delta is not None and self._delta[0][:3] == (T, H, W), "no delta buffer of this shape"
        return self._delta[1][:4 * T * 16 * H * W].view(torch.float32).view(1, T, 16, H, W)

    def step_branch(self, x32, t32, cond: Dict, elem: int, ref, pose, cos, sin, mode=None, n_char: int = 1, cache=None) -> torch.Tensor:
        """One branch of the CFG pair as an evaluation (scail_dit_step_branch): x32 (1,T,16,H,W), t32 (1,), under element ``elem`` of the
        conditioning ``cond`` (any batch).  ``mode``: None, or "fill" / "reuse" on slot ``elem`` of the step cache of the PAIR -- the one this
        object keeps for (2, T, H, W), or a caller-owned uint8 tensor ``cache`` of at least step_cache_bytes(2, T, H, W)."""
        if mode is not None and mode not in L.CACHE_MODES:
            raise L.ScailHipError(f"step_branch: mode must be None or one of {sorted(L.CACHE_MODES)}, got {mode!r}")
        B, T, _, H, W = x32.shape
        if B != 1 or t32.numel() != 1:
            raise L.ScailHipError(f"step_branch: a branch is ONE latent and ONE timestep, got batch {B} and {t32.numel()} timestep(s)")
        if mode is not None and cache is None:
            cache = self._cache_for(2, T, H, W, x32.device, mode == "fill")
        ws = self._ws_for(self.workspace_bytes(1, T, H, W, n_char), x32.device, "scail_dit_chars_workspace_bytes")
        cc = _cond_struct(cond)
        out = torch.empty(1, T, 16, H, W, device=x32.device, dtype=torch.float32)
        assert ref.shape[0] == 1 and pose.shape[0] == 1
        L.call("scail_dit_step_branch", self._h, x32.data_ptr(), t32.data_ptr(), C.byref(cc), cond["k_text"].shape[1], int(elem), ref.data_ptr(),
               pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), out.data_ptr(), T, H, W, ws.data_ptr(), ws.numel(),
               0 if mode is None else L.CACHE_MODES[mode], None if cache is None else cache.data_ptr(), 0 if cache is None else cache.numel(),
               torch.cuda.current_stream().cuda_stream)
        return out

    def sample_guided(self, x32, sigmas, cfg_scale, cond: Dict, ref, pose, cos, sin, guide, reuse=None, n_char: int = 1) -> torch.Tensor:
        """``sample`` under a guidance plan (scail_dit_sample_guided): ``guide`` = one entry per step out of lib.GUIDE_PAIR / _DELTA / _COND
        (sampler.plan_guidance); ``reuse``: None, or the step cache's 0 / 1 plan (sampler.merge_guidance_with_step_cache makes the two
        agree).  Still ONE call that only enqueues.  A plan of COND entries alone takes no delta buffer."""
        _, T, _, H, W = x32.shape
        ts, dsa, n = self._schedule(sigmas, x32.device)
        guide = [int(v) for v in guide]
        if len(guide) != n:
            raise L.ScailHipError(f"sample_guided: the guidance plan needs one entry per step ({n}), got {len(guide)}")
        if any(v < 0 or v > 255 for v in guide):
            raise L.ScailHipError(f"sample_guided: the guidance plan holds entries 0 / 1 / 2, got {guide}")
        if reuse is not None:
            reuse = [int(v) for v in reuse]
            if len(reuse) != n:
                raise L.ScailHipError(f"sample_guided: the reuse mask needs one entry per step ({n}), got {len(reuse)}")
            if any(v < 0 or v > 255 for v in reuse):
                raise L.ScailHipError(f"sample_guided: the reuse mask holds 0 / 1 entries, got {reuse}")
        delta = self._delta_for(T, H, W, x32.device) if any(v != L.GUIDE_COND for v in guide) else None
        cache = self._cache_for(2, T, H, W, x32.device, True) if reuse is not None else None
        ws = self._ws_for(L.load().scail_dit_sample_chars_workspace_bytes(self._h, T, H, W, n_char), x32.device,
                          f"scail_dit_sample_chars_workspace_bytes (T {T}, H {H}, W {W}, n_char {n_char})")
        cc = _cond_struct(cond)
        assert x32.is_contiguous() and x32.dtype == torch.float32 and ref.shape[0] == 1 and pose.shape[0] == 1
        L.call("scail_dit_sample_guided", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale),
               C.byref(cc), ref.data_ptr(), pose.data_ptr(), n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), T, H, W,
               ws.data_ptr(), ws.numel(), (C.c_uint8 * max(n, 1))(*guide), None if delta is None else delta.data_ptr(),
               0 if delta is None else delta.numel(), None if reuse is None else (C.c_uint8 * max(n, 1))(*reuse),
               None if cache is None else cache.data_ptr(), 0 if cache is None else cache.numel(), torch.cuda.current_stream().cuda_stream)
        return x32

    def time_distances(self, timesteps, signal: str = "time") -> torch.Tensor:
        """scail_dit_time_distances: for the device fp32 ``timesteps`` (n,) (= 1000 sigma_i) the (n, 2) fp64 CPU table of
        (sum |v_i - v_{i-1}|, sum |v_{i-1}|) between consecutive steps' time embeddings ("time") or their AdaLN projections ("modulation");
        row 0 is (0, 0).  One host synchronisation (the copy of the table)."""
        if signal not in L.CACHE_SIGNALS:
            raise L.ScailHipError(f"time_distances: signal must be one of {sorted(L.CACHE_SIGNALS)}, got {signal!r}")
        sg = L.CACHE_SIGNALS[signal]
        assert timesteps.is_cuda and timesteps.dtype == torch.float32 and timesteps.dim() == 1 and timesteps.is_contiguous()
        n, dev = timesteps.numel(), timesteps.device
        need = L.load().scail_dit_time_distances_bytes(self._h, sg)
        if need < 0:
            raise L.ScailHipError(f"scail_dit_time_distances_bytes: bad signal {sg}")
        scratch = torch.empty(need, device=dev, dtype=torch.uint8)
        out = torch.empty(max(n, 1), 2, device=dev, dtype=torch.float64)
        L.call("scail_dit_time_distances", self._h, timesteps.data_ptr(), n, sg, out.data_ptr(), scratch.data_ptr(), scratch.numel(),
               torch.cuda.current_stream(dev).cuda_stream)
        return out[:n].cpu()

    def sample_tiled_workspace_bytes(self, T, Tt, H, W) -> int:
        n = L.load().scail_dit_sample_tiled_workspace_bytes(self._h, T, Tt, H, W)
        if n < 0:
            raise L.ScailHipError(f"scail_dit_sample_tiled_workspace_bytes: bad shape (T {T}, Tt {Tt}, H {H}, W {W})")
        return n

    @staticmethod
    def tile_tables(tile_indices, tile_w, inv_wsum):
        """The host arrays of scail_dit_sample_tiled: (tile_frames int32 [n_tiles][Tt], tile_w fp32 [n_tiles][Tt], inv_wsum fp32 [T])."""
        fr = [int(f) for t in tile_indices for f in t]
        tw = tile_w.detach().cpu().float().reshape(-1).tolist()
        iw = inv_wsum.detach().cpu().float().reshape(-1).tolist()
        return (C.c_int32 * len(fr))(*fr), (C.c_float * len(tw))(*tw), (C.c_float * len(iw))(*iw)

    def sample_tiled(self, x32, sigmas, cfg_scale, cond: Dict, ref, pose_tiles, tile_indices, tile_w, inv_wsum, cos, sin, solver=None) -> torch.Tensor:
        """The whole RFSamplerLong loop in one C call (scail_dit_sample_tiled).  x32 (1,T,16,H,W) fp32 is updated in place and returned;
        ``pose_tiles`` bf16 (1, n_tiles, Tt, 16, H/2, W/2); ``tile_indices`` n_tiles lists of Tt frame indices; ``tile_w`` host fp32
        (n_tiles, Tt) = m_k * tile_weight; ``inv_wsum`` host fp32 (T); cos / sin: the tables of a Tt-frame clip.
        ``solver``: None, or ``sample``'s (sigma, coef): the loop under a solver plan (scail_dit_sample_tiled_solver), with one history of
        the full latent."""
        _, T, _, H, W = x32.shape
        n_tiles = len(tile_indices)
        Tt = len(tile_indices[0]) if n_tiles else 0
        hist = self._hist_for(T, H, W, x32.device) if solver is not None else None
        ws = self._ws_for(self.sample_tiled_workspace_bytes(T, Tt, H, W), x32.device, "scail_dit_sample_tiled_workspace_bytes")
        ts, dsa, n = self._schedule(sigmas, x32.device)
        fr, tw, iw = self.tile_tables(tile_indices, tile_w, inv_wsum)
        cc = _cond_struct(cond)
        assert x32.is_contiguous() and x32.dtype == torch.float32 and ref.shape[0] == 1 and pose_tiles.is_contiguous()
        assert pose_tiles.shape == (1, n_tiles, Tt, 16, H // 2, W // 2) and pose_tiles.dtype == torch.bfloat16
        if solver is not None:
            sg, co = self.solver_tables(solver, n)
            L.call("scail_dit_sample_tiled_solver", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale), C.byref(cc),
                   ref.data_ptr(), pose_tiles.data_ptr(), fr, tw, iw, n_tiles, T, Tt, cos.data_ptr(), sin.data_ptr(), H, W,
                   ws.data_ptr(), ws.numel(), sg, co, hist.data_ptr(), hist.numel(), torch.cuda.current_stream().cuda_stream)
            return x32
        L.call("scail_dit_sample_tiled", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale), C.byref(cc),
               ref.data_ptr(), pose_tiles.data_ptr(), fr, tw, iw, n_tiles, T, Tt, cos.data_ptr(), sin.data_ptr(), H, W,
               ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return x32

    def sample_tiled_cache_bytes(self, n_tiles, Tt, H, W) -> int:
        n = L.load().scail_dit_sample_tiled_cache_bytes(self._h, n_tiles, Tt, H, W)
        if n < 0:
            raise L.ScailHipError(f"scail_dit_sample_tiled_cache_bytes: bad shape (n_tiles {n_tiles}, Tt {Tt}, H {H}, W {W})")
        return n

    def _tile_cache_for(self, n_tiles, Tt, H, W, device) -> torch.Tensor:
        """The cache of sample_tiled_cached -- one residual slab per tile and one shared embedding region --, a new one when the tiling,
        the shape or the device changed.  Handed out by ``_ws_for`` and kept beside the workspace, as ``_cache_for`` does."""
        key = (n_tiles, Tt, H, W, torch.device(device))
        if self._tile_cache is None or self._tile_cache[0] != key:
            ws, self._ws = self._ws, None
            try:
                buf = self._ws_for(self.sample_tiled_cache_bytes(n_tiles, Tt, H, W), device,
                                   f"scail_dit_sample_tiled_cache_bytes (n_tiles {n_tiles}, Tt {Tt}, H {H}, W {W})")
            finally:
                self._ws = ws
            self._tile_cache = (key, buf)
        return self._tile_cache[1]

    def tile_cache_residual(self, k, n_tiles, Tt, H, W, D) -> torch.Tensor:
        """tile k's r (2, Lnoise, D) bf16 as the last computed step of sample_tiled_cached left it: a view of slab k of the cache (slabs
        of 2 * Lnoise * D * 2 bytes rounded up to 256, from offset 0)"""
        assert self._tile_cache is not None and self._tile_cache[0][:4] == (n_tiles, Tt, H, W), "no tiled cache of this shape"
        assert 0 <= k < n_tiles
        n = 2 * Tt * (H // 2) * (W // 2) * D
        slab = (2 * n + 255) // 256 * 256
        return self._tile_cache[1][k * slab:k * slab + 2 * n].view(torch.bfloat16).view(2, -1, D)

    def sample_tiled_cached(self, x32, sigmas, cfg_scale, cond: Dict, ref, pose_tiles, tile_indices, tile_w, inv_wsum, cos, sin, reuse) -> torch.Tensor:
        """``sample_tiled`` with a step cache (scail_dit_sample_tiled_cached): ``reuse`` = one 0 / 1 per step, shared by every tile; at a
        step planned 1 every tile reuses its own residual of the last computed step.  Still ONE call that only enqueues.  A call the
        library refuses leaves this object with the tiled cache it had before."""
        _, T, _, H, W = x32.shape
        n_tiles = len(tile_indices)
        Tt = len(tile_indices[0]) if n_tiles else 0
        ts, dsa, n = self._schedule(sigmas, x32.device)
        reuse = [int(v) for v in reuse]
        if len(reuse) != n:
            raise L.ScailHipError(f"sample_tiled_cached: the reuse mask needs one entry per step ({n}), got {len(reuse)}")
        if any(v < 0 or v > 255 for v in reuse):
            raise L.ScailHipError(f"sample_tiled_cached: the reuse mask holds 0 / 1 entries, got {reuse}")
        assert x32.is_contiguous() and x32.dtype == torch.float32 and ref.shape[0] == 1 and pose_tiles.is_contiguous()
        assert pose_tiles.shape == (1, n_tiles, Tt, 16, H // 2, W // 2) and pose_tiles.dtype == torch.bfloat16
        held = self._tile_cache
        try:
            cache = self._tile_cache_for(n_tiles, Tt, H, W, x32.device)
            ws = self._ws_for(self.sample_tiled_workspace_bytes(T, Tt, H, W), x32.device, "scail_dit_sample_tiled_workspace_bytes")
            fr, tw, iw = self.tile_tables(tile_indices, tile_w, inv_wsum)
            cc = _cond_struct(cond)
            L.call("scail_dit_sample_tiled_cached", self._h, x32.data_ptr(), ts.data_ptr(), C.cast(dsa, C.c_void_p), n, float(cfg_scale),
                   C.byref(cc), ref.data_ptr(), pose_tiles.data_ptr(), fr, tw, iw, n_tiles, T, Tt, cos.data_ptr(), sin.data_ptr(), H, W,
                   ws.data_ptr(), ws.numel(), (C.c_uint8 * max(n, 1))(*reuse), cache.data_ptr(), cache.numel(),
                   torch.cuda.current_stream().cuda_stream)
        except L.ScailHipError:
            self._tile_cache = held
            raise
        return x32

    def block(self, layer: int, hidden: torch.Tensor, mod: torch.Tensor, cond: Dict, cos, sin) -> torch.Tensor:
        """Seam B2: one transformer block in place on ``hidden`` (B, Ltok, D) bf16; ``mod`` (B, 6D) fp32 = adaLN embedding +
        this layer's table.  Returns ``hidden``."""
        B, Ltok, _ = hidden.shape
        ws = self._ws_for(L.load().scail_dit_block_workspace_bytes(self._h, B, Ltok), hidden.device,
                          f"scail_dit_block_workspace_bytes (B {B}, Ltok {Ltok})")
        cc = _cond_struct(cond)
        assert hidden.is_contiguous() and mod.is_contiguous() and mod.dtype == torch.float32
        L.call("scail_dit_block", self._h, layer, hidden.data_ptr(), mod.data_ptr(), C.byref(cc), cos.data_ptr(), sin.data_ptr(),
               B, Ltok, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return hidden

    # ---- sequence-parallel rank (include/scail_dit.h: scail_dit_step_sp / scail_dit_block_sp) ----
    def _sp_call(self, name, xch, *args):
        """Run one executor call whose collectives go through ``xch`` (scail_amd.parallel.CExchange); an exception raised inside the
        callback is re-raised here (the executor only sees a non-zero status)."""
        xch.error = None
        try:
            L.call(name, *args)
        except L.ScailHipError:
            if xch.error is not None:
                raise xch.error
            raise

    def step_sp(self, x32, t32, cond: Dict, ref, pose, cos, sin, xch, cfg_pair: bool = False, n_char: int = 1) -> torch.Tensor:
        """One network evaluation on this rank's latent slab (scail_dit_step_sp_chars); ``xch`` owns the exchange buffers and issues the
        collectives from the executor's callback.  ``ref`` / ``pose`` are the rank's slabs of all ``n_char`` characters."""
        B, T, _, H, W = x32.shape
        ws = self._ws_for(L.load().scail_dit_sp_chars_workspace_bytes(self._h, xch.mode_code, xch.size, B, T, H, W, n_char), x32.device,
                          f"scail_dit_sp_chars_workspace_bytes (mode {xch.mode_code}, {xch.size} ranks, B {B}, T {T}, H {H}, W {W}, n_char {n_char})")
        cc, sp = _cond_struct(cond), xch.descriptor()
        out = torch.empty(B, T, 16, H, W, device=x32.device, dtype=torch.float32)
        self._sp_call("scail_dit_step_sp_chars", xch, self._h, x32.data_ptr(), t32.data_ptr(), C.byref(cc), ref.data_ptr(), ref.shape[0],
                      pose.data_ptr(), pose.shape[0], n_char, pose.shape[1], cos.data_ptr(), sin.data_ptr(), out.data_ptr(), B, T, H, W, C.byref(sp),
                      self.CFG_PAIR if cfg_pair else 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return out

    def block_sp(self, layer: int, hidden: torch.Tensor, mod: torch.Tensor, cond: Dict, cos, sin, xch) -> torch.Tensor:
        """Seam B2 for a sequence-parallel rank: one block in place on this rank's ``hidden`` (B, Ltok, D)."""
        B, Ltok, _ = hidden.shape
        ws = self._ws_for(L.load().scail_dit_block_sp_workspace_bytes(self._h, xch.mode_code, xch.size, B, Ltok), hidden.device,
                          f"scail_dit_block_sp_workspace_bytes (mode {xch.mode_code}, {xch.size} ranks, B {B}, Ltok {Ltok})")
        cc, sp = _cond_struct(cond), xch.descriptor()
        assert hidden.is_contiguous() and mod.is_contiguous() and mod.dtype == torch.float32
        self._sp_call("scail_dit_block_sp", xch, self._h, layer, hidden.data_ptr(), mod.data_ptr(), C.byref(cc), cos.data_ptr(), sin.data_ptr(),
                      B, Ltok, C.byref(sp), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return hidden
