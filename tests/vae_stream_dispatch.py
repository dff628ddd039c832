"""Host-side walk of the decoder's launches (csrc/vae_exec.hip decode_frames) that names, for every launch, the kernel the dispatch of
csrc/conv.hip conv3d_impl / csrc/gemm.hip picks for its geometry.  The streamed decode (scail_vae_decode_stream) computes every output voxel
from the same inputs as the whole-sequence decode; the two are bit-identical only where each launch picks the same kernel for the chunk's
geometry as for the clip's.  tests/test_vae_stream_gpu.py asserts that precondition with this walk before it compares bits, so that a
mismatch reads as a dispatch difference and not as wrong arithmetic.

Every convolution's kernel is the library's own word: scail_conv3d_kernel_name_for names the kernel csrc/conv.hip picks (conv_choose, the
rule its launches follow), scail_conv3d_norm_fused_for says how a ResidualBlock runs residual.2.  No threshold, shape table or kernel order of
the convolutions is restated here (the GEMM's still is, in _gemm).  Needs no GPU."""
import ctypes as C


def _conv(lib, Cin, N, k, Ti, To, H, W, pt, resid=False, ups=False, fuse=None, ot_mul=1, ot_off=0):
    """the kernel of one convolution launch; fuse: None plain, "norm" residual.2 of a ResidualBlock, "dual" scail_conv3d_cl_resid_norm"""
    from scail_amd import lib as L
    kt, kh, kw = k
    Cin, N = (Cin + 7) // 8 * 8, (N + 7) // 8 * 8
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    kpad = (kt * kh * kw * Cin + 63) // 64 * 64
    geom = C.cast((C.c_int32 * 21)(Ti, H, W, Cin, To, Ho, Wo, kt, kh, kw, 1, 1, 1, pt, kh // 2, kw // 2, int(ups), ot_mul, ot_off, N, kpad), C.c_void_p)
    form = 2 if fuse == "dual" else 1 if fuse == "norm" and lib.scail_conv3d_norm_fused_for(geom, N) else 0
    buf = C.create_string_buffer(128)
    L.call("scail_conv3d_kernel_name_for", geom, N, N if resid else 0, form, buf, len(buf))
    return buf.value.decode()


def _gemm(lib, M, N, K, resid=False):
    k = lib.scail_gemm_kernel_for(K, N, N if resid else 0, M, N, K, 3 if resid else 0)
    return ("gemm generated",) if k else ("gemm", M >= 2048 and N >= 1024)


def decoder_launches(model, n, hl, wl, first=True):
    """[(name, kernel)] of one pass of the decoder over ``n`` latent frames of hl x wl: the whole clip or a streamed decode's first chunk
    (first=True: causal padding, frame 0 bypasses the time convolutions) or a later chunk (every causal convolution reads two carried
    frames in front of the chunk, pt = 0)."""
    from scail_amd import lib as L
    lib = L.load()
    out = []

    def causal(name, Cin, N, T, H, W, **kw):
        out.append((name, _conv(lib, Cin, N, (3, 3, 3), T if first else T + 2, T, H, W, 2 if first else 0, **kw)))

    def res(name, cin, cout, T, H, W, nxt):
        if cin != cout:
            out.append((name + ".shortcut", _conv(lib, cin, cout, (1, 1, 1), T, T, H, W, 0)))
        causal(name + ".residual.2", cin, cout, T, H, W, fuse="norm")
        causal(name + ".residual.6", cout, cout, T, H, W, resid=True, fuse="dual" if nxt else None)

    z, top, T, H, W = model.z_dim, model.dim * model.dim_mult[-1], n, hl, wl
    out.append(("conv2", _conv(lib, z, z, (1, 1, 1), T, T, H, W, 0)))
    causal("decoder.conv1", z, top, T, H, W)
    res("decoder.middle.0", top, top, T, H, W, False)
    for nm in "qkv":
        out.append(("decoder.middle.1." + nm, _gemm(lib, T * H * W, top, top)))
    out.append(("decoder.middle.1.proj", _gemm(lib, T * H * W, top, top, resid=True)))
    res("decoder.middle.2", top, top, T, H, W, False)
    plan = model.decoder_plan()
    for i, (kind, name, a, b) in enumerate(plan):
        if kind == "res":
            res(name, a, b, T, H, W, i + 1 == len(plan) or plan[i + 1][0] == "res")
            continue
        if b and (T > 1 or not first):
            tail = T - 1 if first else T
            for p in (0, 1):
                out.append((f"{name}.time_conv#{p}", _conv(lib, a, a, (3, 1, 1), tail if first else tail + 2, tail, H, W, 2 if first else 0,
                                                           ot_mul=2, ot_off=(1 if first else 0) + p)))
            T = (1 if first else 0) + 2 * tail
        nxt = i + 1 < len(plan) and plan[i + 1][0] == "res"
        out.append((name + ".resample", _conv(lib, a, a // 2, (1, 3, 3), T, T, H, W, 0, ups=True, fuse="dual" if nxt else None)))
        H, W = 2 * H, 2 * W
    causal("decoder.head.2", model.dim, 3, T, H, W)
    return out


def chunk_plan(Tl, chunk):
    """[(first latent frame, frames)] of scail_vae_decode_stream: chunks of ``chunk``, a remainder of one frame joins the last chunk; one chunk
    when Tl <= chunk + 1"""
    if Tl <= chunk + 1:
        return [(0, Tl)]
    plan, t0 = [], 0
    while t0 < Tl:
        n = min(chunk, Tl - t0)
        if Tl - t0 - n == 1:
            n += 1
        plan.append((t0, n))
        t0 += n
    return plan


def dispatch_differences(model, Tl, hl, wl, chunk):
    """launches of a streamed decode whose kernel differs from the whole-sequence decode's: [(chunk start, name, chunk kernel, whole kernel)]"""
    whole = dict(decoder_launches(model, Tl, hl, wl))
    plan = chunk_plan(Tl, chunk)
    if len(plan) == 1:
        return []
    diffs = []
    for t0, n in plan:
        for name, k in decoder_launches(model, n, hl, wl, first=t0 == 0):
            if whole.get(name) != k:
                diffs.append((t0, name, k, whole.get(name)))
    return diffs
