"""Wiring tests of the conditioning encoders on the GPU: every route through scail_amd/umt5.py and scail_amd/clip.py runs the PLANTED
towers on the planted inputs (tests/enc_wiring.py) and is compared with the fp32 oracle by e(a, b) = ||a - b||_2 / ||b||_2 at every
observation point the route exposes.  The bound at point p is T_p = 2 N_p, N_p being the distance of the CPU bf16-storage model from
the oracle (enc_wiring.t5_bounds / clip_bounds: derived on the CPU, proven discriminating by tests/test_enc_wiring_cpu.py -- every
catalogue mutant moves some point by >= 4 T_p or is exempt with its proof -- and never taken from a GPU result).  A value over T_p is a
finding: a store point the model misses, or a wrong wire.

Every test prints its figures (route, point, N_p, T_p, measured) before it asserts; profiles/enc_wiring.log is that output."""
import os

import numpy as np
import pytest
import torch

import enc_wiring as W
from oracle import encoders_oracle as E

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t5():
    from scail_amd.umt5 import T5Encoder
    enc = T5Encoder(shared_pos=False, device=DEV, **W.T5CFG)
    missing, unexpected = enc.load_state_dict(W.planted_t5(), strict=True)
    assert not missing and not unexpected
    return enc


def _vit_kw():
    return dict(W.VITCFG)


def _vit():
    from scail_amd.clip import VisionTransformer
    vit = VisionTransformer(device=DEV, **_vit_kw())
    missing, unexpected = vit.load_state_dict(W.planted_vit(), strict=True)
    assert not missing and not unexpected
    return vit


def _tapped(net):
    """the observation points of a tower through its _tap hook (the stream is updated in place: every tap is copied)"""
    taps = {}
    net._tap = lambda i, h: taps.__setitem__("x0" if i < 0 else f"h{i + 1}", h.float().cpu().clone())
    return taps


@pytest.fixture(scope="module")
def t5():
    """weights, inputs, the oracle's observation points (computed once, never written to) and the CPU-derived bounds; the same with a
    mask of ones"""
    sd = W.planted_t5()
    out = {}
    for full in (False, True):
        inp = W.planted_t5_inputs(full_mask=full)
        out[full] = dict(inp=inp, ref=W.t5_points(W.T5CFG, sd, inp), bounds=W.t5_bounds(full))
    return out


@pytest.fixture(scope="module")
def vit():
    sd, imgs = W.planted_vit(), W.planted_images()
    return dict(sd=sd, imgs=imgs, ref=W.clip_points(W.VITCFG, sd, imgs), bounds=W.clip_bounds())


def _check(capsys, route, bounds, got, want, T=None):
    """print every figure of the route, then assert all of them"""
    rows = [(p, bounds["N"][p], (T or bounds["T"])[p], W.e(got[p].float().cpu(), want[p])) for p in got]
    with capsys.disabled():
        print()
        for p, n, t, m in rows:
            print("wiring  %-46s %-6s N_p %.3e  T_p %.3e  measured %.3e  (%s N_p)%s"
                  % (route, p, n, t, m, "%.2f" % (m / n) if n else "-", "" if m <= t else "   OVER"))
    over = [(p, m, t) for p, _, t, m in rows if not m <= t]
    assert not over, f"{route}: over T_p at {over}"


def test_t5_encoder_batch(t5, capsys):
    """T5Encoder.forward on the planted batch (valid lengths 136, 51, 1), hidden states through _tap"""
    c, enc = t5[False], _t5()
    taps = _tapped(enc)
    out = enc(c["inp"]["ids"].to(DEV), c["inp"]["mask"].to(DEV))
    assert set(taps) == {"x0", "h1", "h2"} and out.dtype == torch.bfloat16
    _check(capsys, "T5Encoder.forward (B = 3)", c["bounds"], dict(taps, out=out), c["ref"])


@pytest.mark.parametrize("row", range(W.B))
def test_t5_encoder_one_row(t5, capsys, row):
    """the same rows one at a time: the same bounds"""
    c, enc = t5[False], _t5()
    taps = _tapped(enc)
    out = enc(c["inp"]["ids"][row:row + 1].to(DEV), c["inp"]["mask"][row:row + 1].to(DEV))
    want = {p: v[row:row + 1] for p, v in c["ref"].items()}
    _check(capsys, f"T5Encoder.forward (B = 1, row {row}: {W.VALID[row]} valid)", c["bounds"], dict(taps, out=out), want)


def test_t5_encoder_without_a_mask(t5, capsys):
    """mask = None against the oracle with a mask of ones"""
    c, enc = t5[True], _t5()
    assert bool(c["inp"]["mask"].all()) and not torch.equal(c["ref"]["out"], t5[False]["ref"]["out"])
    taps = _tapped(enc)
    out = enc(c["inp"]["ids"].to(DEV), None)
    _check(capsys, "T5Encoder.forward (mask = None)", c["bounds"], dict(taps, out=out), c["ref"])


def test_t5_encoder_model_zeroes_the_padded_rows(t5, capsys):
    """T5EncoderModel.forward: padded rows exactly zero, valid rows within T_out"""
    from scail_amd.umt5 import T5EncoderModel
    c = t5[False]
    m = T5EncoderModel(max_length=W.LEN, device=DEV, shared_pos=False, **W.T5CFG)
    missing, unexpected = m.model.load_state_dict(W.planted_t5(), strict=True)
    assert not missing and not unexpected
    z = m(c["inp"]["ids"].to(DEV), c["inp"]["mask"].to(DEV)).float().cpu()
    valid = c["inp"]["mask"].bool()
    b = c["bounds"]
    got = {"model": z, "out": z[valid]}
    want = {"model": c["ref"]["model"], "out": c["ref"]["out"][valid]}
    with capsys.disabled():
        print("\nwiring  T5EncoderModel.forward: largest |value| in the %d padded rows: %g" % (int((~valid).sum()), float(z[~valid].abs().max())))
    _check(capsys, "T5EncoderModel.forward (out: valid rows only)", b, got, want, T={"model": b["T"]["model"], "out": b["T"]["out"]})
    assert float(z[~valid].abs().max()) == 0 and int((~valid).sum()) == 3 * 136 - 188


def test_vit_batch(vit, capsys):
    """VisionTransformer.forward(use_31_block=True) on the three planted images"""
    net = _vit()
    taps = _tapped(net)
    out = net(vit["imgs"].to(DEV), use_31_block=True)
    assert set(taps) == {"x0", "h1", "h2"} and out.shape == (3, 26, 320)
    _check(capsys, "VisionTransformer.forward (B = 3)", vit["bounds"], dict(taps, out=out), vit["ref"])


@pytest.mark.parametrize("image", range(W.B))
def test_vit_one_image(vit, capsys, image):
    net = _vit()
    taps = _tapped(net)
    out = net(vit["imgs"][image:image + 1].to(DEV), use_31_block=True)
    want = {p: v[image:image + 1] for p, v in vit["ref"].items()}
    _check(capsys, f"VisionTransformer.forward (B = 1, image {image})", vit["bounds"], dict(taps, out=out), want)


def test_clip_model_visual(vit, golden_dir, capsys):
    """CLIPModel.visual on one 3 x 1 x 96 x 160 clip through the planted tower (image_size 70): its preprocessing against the real
    reference's (tests/golden/encoders_planted.npz "pre"), its output against clip_preprocess + the oracle, and the tower on the golden
    preprocessing against the oracle on the same, both at the tower's T_out.

    The bound on the preprocessing is 4 x the distance of torch's CPU bicubic (E.clip_preprocess) from the golden -- but that distance
    is exactly 0 here (the golden IS torch's CPU bicubic, run by the reference's code), and a bound of 0 would ask the GPU for the CPU's
    bits.  So the distance is floored by what fp32 allows the operation (enc_wiring.pre_floor: 2^-21) before the 4 x."""
    from scail_amd.clip import CLIPModel
    with np.load(os.path.join(golden_dir, "encoders_planted.npz")) as z:
        gpre = torch.from_numpy(np.asarray(z["pre"]))
    clip = W.planted_clip()
    cpu_pre = W.pre_points(clip)["pre"]
    e_cpu = W.e(cpu_pre, gpre)
    t_pre = 4.0 * max(e_cpu, W.pre_floor())
    m = CLIPModel(device=DEV, **_vit_kw())
    missing, unexpected = m.model.visual.load_state_dict(W.planted_vit(), strict=True)
    assert not missing and not unexpected
    seen = []
    hook = m.model.visual.register_forward_pre_hook(lambda mod, args: seen.append(args[0].float().cpu().clone()))
    feats = m.visual([clip.to(DEV)])
    hook.remove()
    assert len(seen) == 1 and seen[0].shape == gpre.shape == (1, 3, 70, 70)
    e_pre = W.e(seen[0], gpre)
    with capsys.disabled():
        print("\nwiring  CLIPModel.visual preprocessing            pre    CPU torch bicubic against the golden %.3e  floor %.3e  bound %.3e  measured %.3e%s"
              % (e_cpu, W.pre_floor(), t_pre, e_pre, "" if e_pre <= t_pre else "   OVER"))
    b, cfg = vit["bounds"], W.VITCFG
    want = W.clip_points(cfg, vit["sd"], cpu_pre)
    _check(capsys, "CLIPModel.visual (clip_preprocess + oracle)", b, dict(out=feats), want)
    on_golden = m.model.visual(gpre.to(DEV), use_31_block=True)
    _check(capsys, "VisionTransformer.forward on the golden pre", b, dict(out=on_golden), W.clip_points(cfg, vit["sd"], gpre))
    assert e_pre <= t_pre, (e_pre, t_pre)
