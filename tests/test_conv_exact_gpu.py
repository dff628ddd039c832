"""Every convolution kernel csrc/conv.hip can pick -- the five hipcc templates and the eleven generated entry points of conv4.s / conv4u.s -- on
operands for which fp32 accumulation is exact in any order (tests/conv_exact.py): the plain and residual epilogues bit for bit against the fp64
convolution + bias (+ residual) rounded once to bf16, the norm epilogues (scail_rms_silu, scail_conv3d_cl_norm, scail_conv3d_cl_resid_norm) correctly
rounded wherever fp32 arithmetic can decide it (check_rounded_bf16 with the derived MARGIN).  Every case first asserts the kernel it runs by name
(scail_conv3d_kernel_name_for), writes into NaN-filled tensors -- row stride above N and interleaved output frames where the call takes them, a guard
frame behind the dense outputs of the norm calls -- and asserts that nothing else was written.  tests/test_conv_exact_cpu.py proves that these
checks reject a truncating pack, a dropped (tap, channel) pair, a bias added after the rounding, sqrt(C - 1) and a norm of the unrounded sum."""
import ctypes as C

import pytest
import torch

import conv_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _case(id):
    return next(c for c in E.PLAIN_CASES + E.NORM_CASES + E.RESID_NORM_CASES if c["id"] == id)


def _ids(cases):
    return [c["id"] for c in cases]


def _device_operands(case):
    """x channels-last with Cin padded to a multiple of 8, the prepared weights (N = cout padded to 8), and the padded fp32 weight / bias the reference uses"""
    from scail_amd import ops
    o = E.operands(case)
    cin, cout = case["cin"], case["cout"]
    cpad, N = (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
    x = torch.zeros(tuple(case["thw"]) + (cpad,), dtype=torch.bfloat16)
    x[..., :cin] = o["x"].permute(1, 2, 3, 0).to(torch.bfloat16)
    wp = ops.prep_conv_weight(o["w"].to(DEV), o["bias"].to(DEV), cin_pad=cpad)
    assert wp["N"] == N
    wN = torch.zeros((N,) + tuple(o["w"].shape[1:]))
    wN[:cout] = o["w"]
    bN = torch.zeros(N)
    bN[:cout] = o["bias"]
    return o, x.to(DEV), wp, wN, bN, N


@pytest.mark.parametrize("id", _ids(E.PLAIN_CASES))
def test_plain_and_residual_epilogues_bit_exact(id):
    from scail_amd import ops
    case = _case(id)
    o, x, wp, wN, bN, N = _device_operands(case)
    To, Ho, Wo = E.out_thw(case)
    frames, ldc, ldr = 2 * To + 1, N + 32, N + 8                       # results in slots 1, 3, .. of a wider tensor
    geo = dict(stride=case["stride"], pad=case["pad"], ups=case["ups"])
    resid = torch.full((frames, Ho, Wo, ldr), NAN, dtype=torch.bfloat16)      # NaN wherever the kernel has no business reading
    if case["resid"] is not None:
        resid[1::2, :, :, :N] = o["resid"].to(torch.bfloat16)

    def run():
        assert E.kernel_name(case, 0, ldc, 0, 2, 1) == case["plain"]
        out = torch.full((frames, Ho, Wo, ldc), NAN, dtype=torch.bfloat16, device=DEV)
        ops.conv3d_cl(x, wp, (To, Ho, Wo), out=out, ot_mul=2, ot_off=1, **geo)
        out_r = None
        if case["resid"] is not None:
            assert E.kernel_name(case, 0, ldc, ldr, 2, 1) == case["resid"]
            out_r = torch.full((frames, Ho, Wo, ldc), NAN, dtype=torch.bfloat16, device=DEV)
            ops.conv3d_cl(x, wp, (To, Ho, Wo), out=out_r, ot_mul=2, ot_off=1, resid=resid.to(DEV), **geo)
        torch.cuda.synchronize()
        return out, out_r

    out, out_r = E.with_options(case["opts"], run)
    E.assert_bits(out.cpu(), E.conv_ref(o["x"], wN, bN, None, ot_mul=2, ot_off=1, frames=frames, ldc=ldc, **geo), f"{id}: {case['plain']}")
    if case["cout"] < N:
        assert float(out[1::2, :, :, case["cout"]:N].float().abs().max()) == 0.0, "padding channels of the output: exactly zero"
    if out_r is not None:
        E.assert_bits(out_r.cpu(), E.conv_ref(o["x"], wN, bN, o["resid"], ot_mul=2, ot_off=1, frames=frames, ldc=ldc, **geo), f"{id}: {case['resid']}")


def _guarded(To, Ho, Wo, N):
    """a dense output with one NaN guard frame behind it"""
    return torch.full((To + 1, Ho, Wo, N), NAN, dtype=torch.bfloat16, device=DEV)


def _check_norm(what, nrm, ref):
    To = ref.shape[0]
    assert bool(torch.isnan(nrm[To:].float()).all()), f"{what}: written behind the output"
    share = E.check_rounded_bf16(nrm[:To].cpu(), ref, E.MARGIN, what)
    assert share <= E.UNDECIDED_CAP, share


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("Cc", E.RMS_SILU_CHANNELS)
def test_rms_silu_correctly_rounded(Cc, silu):
    from scail_amd import ops
    x, gamma = E.integer_rows(E.RMS_SILU_ROWS, Cc, seed=Cc + (1 if silu else 0))
    s = x.to(torch.bfloat16)
    out = torch.full((E.RMS_SILU_ROWS + 1, Cc), NAN, dtype=torch.bfloat16, device=DEV)
    ops.rms_silu(s.to(DEV), gamma.to(DEV), silu=silu, out=out)
    torch.cuda.synchronize()
    ref = E.norm_silu_ref(s, gamma, silu)
    _check_norm(f"scail_rms_silu C={Cc} silu={silu}", out, ref)
    assert float(out[0].float().abs().max()) == 0.0, "an all-zero row stays zero"


@pytest.mark.parametrize("id", _ids(E.NORM_CASES))
def test_conv_norm_fused_correctly_rounded(id):
    from scail_amd import lib as L
    case = _case(id)
    o, x, wp, wN, bN, N = _device_operands(case)
    To, Ho, Wo = E.out_thw(case)
    gamma = o["gamma"].to(DEV)
    geom = E.geometry(case, N, wp["Kpad"], wp["Cin"])

    def run():
        assert E.kernel_name(case, 1, N, 0) == case["plain"]
        nrm = _guarded(To, Ho, Wo, N)
        L.call("scail_conv3d_cl_norm", x.data_ptr(), wp["w"].data_ptr(), wp["b"].data_ptr(), nrm.data_ptr(), N, gamma.data_ptr(),
               C.cast(geom, C.c_void_p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return nrm

    nrm = E.with_options(case["opts"], run)
    _check_norm(f"{id}: {case['plain']}", nrm, E.norm_reference(case)[1])


def _resid_norm_call(case, x, wp, N, raw, nrm, resid, gamma):
    from scail_amd import lib as L
    geom = E.geometry(case, N, wp["Kpad"], wp["Cin"])
    L.call("scail_conv3d_cl_resid_norm", x.data_ptr(), wp["w"].data_ptr(), wp["b"].data_ptr(), None if raw is None else raw.data_ptr(), nrm.data_ptr(), N,
           None if resid is None else resid.data_ptr(), 0 if resid is None else N, gamma.data_ptr(), C.cast(geom, C.c_void_p),
           torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("id", _ids(E.RESID_NORM_CASES))
def test_conv_resid_next_norm_correctly_rounded(id):
    case = _case(id)
    o, x, wp, wN, bN, N = _device_operands(case)
    To, Ho, Wo = E.out_thw(case)
    gamma = o["gamma"].to(DEV)
    resid = o["resid"].to(torch.bfloat16).to(DEV) if case["with_resid"] else None

    def run():
        assert E.kernel_name(case, 2 if case["want_raw"] else 3, N, N if case["with_resid"] else 0) == case["plain"]
        raw = _guarded(To, Ho, Wo, N) if case["want_raw"] else None
        nrm = _guarded(To, Ho, Wo, N)
        _resid_norm_call(case, x, wp, N, raw, nrm, resid, gamma)
        torch.cuda.synchronize()
        return raw, nrm

    raw, nrm = E.with_options(case["opts"], run)
    s, ref = E.norm_reference(case)
    if raw is not None:
        assert bool(torch.isnan(raw[To:].float()).all()), "written behind the raw output"
        E.assert_bits(raw[:To].cpu(), s, f"{id}: raw sum of {case['plain']}")
    _check_norm(f"{id}: {case['plain']}", nrm, ref)


def test_resid_norm_validates_the_norm_pass_before_launching_the_convolution():
    """576 output channels run as two calls, and scail_rms_silu takes at most 512: the call is refused before the convolution is enqueued"""
    from scail_amd import lib as L
    case = E._c("rn-576", 32, 576, E.K333, (2, 8, 16), "scail_conv4_e0 + scail_rms_silu", want_raw=True, with_resid=False)
    o = E.exact_operands(case["cin"], case["cout"], case["k"], case["thw"], seed=576)
    from scail_amd import ops
    wp = ops.prep_conv_weight(o["w"].to(DEV), o["bias"].to(DEV))
    x = o["x"].permute(1, 2, 3, 0).contiguous().to(torch.bfloat16).to(DEV)
    assert E.kernel_name(case, 2, 576, 0) == case["plain"]
    raw, nrm = _guarded(2, 8, 16, 576), _guarded(2, 8, 16, 576)
    with pytest.raises(L.ScailHipError, match="N <= 512"):
        _resid_norm_call(case, x, wp, 576, raw, nrm, None, torch.ones(576, device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw.float()).all()) and bool(torch.isnan(nrm.float()).all()), "nothing was launched"
