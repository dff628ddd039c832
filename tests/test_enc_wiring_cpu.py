"""The encoders' wiring net, proven on the CPU before anything runs on a GPU (helper and definitions: tests/enc_wiring.py; the scheme is
that of tests/test_dit_wiring_cpu.py).

N_p is the distance e(model, oracle) = ||a - b||_2 / ||b||_2 of the bf16-storage model from the fp32 oracle at observation point p (the
larger of two draws of the inputs); T_p = 2 N_p is the bound tests/test_enc_wiring_gpu.py holds every route of the HIP path to.

  (a) the model is within T_p / 2 on both draws and the draws agree to 25 %; the single rows of the T5 batch (the B = 1 routes of the GPU
      tests) and the single images meet the batch's T_p in the model too.  T5's "x0" is a gather from a bf16 table: N_p = T_p = 0, exact.
  (b) every catalogue entry moves the fp32 oracle by >= 4 T_p at one observation point or more, or is in EXEMPT with its proof: the k third
      of CLIP's to_qkv.bias cancels in the softmax (e <= 1e-5 at every point), and tanh- against erf-GELU stays below T_p at every point
      (tests/gemm_exact.py owns which GELU an epilogue computes).  CLIP's norm_eps is NOT exempt: a planted token shows it.
  (c) for the record, the reason these tests exist: on tests/golden/encoders_tiny.npz every norm-parameter mutant IS the unmutated network
      (its gammas are 1 and its LayerNorm biases 0), and the arithmetic-level mutants pass rtol = atol = 3e-2 in fp32 with no bf16 noise.
  The oracle on the planted towers equals the real reference classes (tests/golden/encoders_planted.npz) at rtol = atol = 1e-4."""
import os

import numpy as np
import pytest
import torch

import enc_wiring as W
from oracle import encoders_oracle as E


def _golden(golden_dir, name):
    out = {}
    with np.load(os.path.join(golden_dir, name)) as z:
        for k in z.files:
            a = torch.from_numpy(np.asarray(z[k]))
            out[k] = a.view(torch.bfloat16).float() if a.dtype == torch.int16 else a
    return out


def test_planted_shapes():
    cfg, sd, inp, points, _ = W.tower("t5")
    assert (cfg["dim"], cfg["dim_attn"], cfg["num_heads"], cfg["dim_ffn"], cfg["num_layers"]) == (128, 192, 3, 320, 2)
    assert cfg["dim_attn"] != cfg["dim"] and cfg["dim_attn"] // cfg["num_heads"] == 64
    assert inp["ids"].shape == (3, 136) and inp["mask"].sum(1).tolist() == [136, 51, 1] and 136 % 64
    bucket = E.t5_bucket(136, 136, 32)
    assert sorted(torch.unique(bucket).tolist()) == [b for b in range(32) if b != W.UNREACHED_BUCKET]        # all 31 reachable buckets
    rel = (torch.arange(136)[None] - torch.arange(136)[:, None]).abs()
    assert int((rel >= 128).sum()) == 72 and set(bucket[rel >= 128].tolist()) == set(W.CLAMP_BUCKETS)         # the clamp is engaged
    valid = inp["mask"].bool()
    assert int((inp["ids"][valid] == W.TINY_ID).sum()) == 10 and not (inp["ids"][~valid] != 0).any() and int(inp["ids"][2, 0]) != W.TINY_ID
    rms = sd["token_embedding.weight"].pow(2).mean(1).sqrt()
    assert abs(float(rms[W.TINY_ID]) - 1e-3) < 1e-5 and float(rms[torch.arange(64) != W.TINY_ID].min()) > 0.3
    pts = points(cfg, sd, inp)
    assert pts["out"].shape == (3, 136, 128) and float(pts["model"][~valid].abs().max()) == 0
    gam = [sd[k] for k in W.T5_GAMMAS]
    assert all(0.5 <= float(g.min()) and float(g.max()) <= 2.0 for g in gam) and all(not torch.equal(gam[0], g) for g in gam[1:])

    cfg, sd, imgs, points, _ = W.tower("clip")
    assert (cfg["dim"], cfg["num_heads"], cfg["num_layers"], cfg["dim"] // cfg["num_heads"]) == (320, 4, 3, 80)
    pts = points(cfg, sd, imgs)
    assert imgs.shape == (3, 3, 70, 70) and pts["out"].shape == (3, 26, 320) and set(pts) == {"x0", "h1", "h2", "out"}
    tok = torch.nn.functional.conv2d(imgs, sd["patch_embedding.weight"], None, stride=14).flatten(2)[W.TINY_IMAGE, :, W.TINY_TOKEN - 1]
    assert float(tok.abs().max()) == 0 and float((tok + sd["pos_embedding"][0, W.TINY_TOKEN]).var()) < 2e-6       # the token that shows norm_eps
    big, small = sd["transformer.2.attn.proj.weight"], sd["transformer.1.attn.proj.weight"]
    assert float(big.std() / small.std()) > 7                                                                    # the block never evaluated
    assert W.planted_clip().shape == W.CLIP_SHAPE and float(W.planted_clip().abs().max()) <= 1
    for t in list(sd.values()) + list(W.planted_t5().values()) + [imgs, W.planted_clip()]:
        assert torch.equal(t, W.bf16r(t))                                                                        # bf16-exact
    assert set(W.planted_t5()) == set(W.t5_spec()) and set(sd) == set(W.vit_spec())


def test_helper_restates_the_oracle():
    """t5_points / clip_points are E.t5_encoder / E.clip_visual_31 bit for bit; the storage models without their roundings are the oracle up
    to fp32 re-association"""
    ident = lambda x: x
    for full in (False, True):
        cfg, sd, inp = W.T5CFG, W.planted_t5(), W.planted_t5_inputs(full_mask=full)
        pts = W.t5_points(cfg, sd, inp)
        assert torch.equal(pts["out"], E.t5_encoder(sd, inp["ids"], inp["mask"], cfg["num_heads"], cfg["num_layers"], cfg["num_buckets"]))
        assert torch.equal(pts["x0"], sd["token_embedding.weight"][inp["ids"]])
        got = W.t5_storage(cfg, sd, inp, r=ident)
        assert set(got) == set(pts) == set(W.T5_POINTS) and all(W.e(got[p], pts[p]) < 5e-6 for p in pts)
    h1 = E.t5_encoder(sd, inp["ids"], inp["mask"], cfg["num_heads"], 1, cfg["num_buckets"])                      # one layer + the final norm
    assert torch.equal(W.t5_final(sd, pts["h1"]), h1)
    cfg, sd, imgs = W.VITCFG, W.planted_vit(), W.planted_images()
    pts = W.clip_points(cfg, sd, imgs)
    assert torch.equal(pts["out"], E.clip_visual_31(sd, imgs, cfg["num_heads"], cfg["num_layers"], cfg["patch_size"], cfg["norm_eps"]))
    assert torch.equal(pts["h2"], pts["out"])
    assert torch.equal(pts["h1"], E.clip_visual_31(sd, imgs, cfg["num_heads"], 2, cfg["patch_size"]))
    assert torch.equal(pts["x0"], E.clip_visual_31(sd, imgs, cfg["num_heads"], 1, cfg["patch_size"]))
    got = W.clip_storage(cfg, sd, imgs, r=ident)
    assert set(got) == set(pts) == set(W.CLIP_POINTS) and all(W.e(got[p], pts[p]) < 5e-6 for p in pts)


def test_a_noise_model_and_bounds(capsys):
    tables = [("t5", W.t5_bounds()), ("t5, mask of ones", W.t5_bounds(True)), ("clip", W.clip_bounds())]
    lines = ["tower / point            N_p (draw 1)  N_p (draw 2)  T_p"]
    for name, b in tables:
        for p in b["N"]:
            lines.append("%-18s %-5s %.3e     %.3e     %.3e" % (name, p, b["draws"][0][p], b["draws"][1][p], b["T"][p]))
    # the rows of the T5 batch one at a time and the images one at a time: the storage model against the oracle, held to the batch's T_p
    cfg, sd, inp, points, b = W.tower("t5")
    single = []
    for r in range(W.B):
        one = {k: v[r:r + 1] for k, v in inp.items()}
        ref, got = points(cfg, sd, one), W.t5_storage(cfg, sd, one)
        single += [("t5 row %d" % r, p, W.e(got[p], ref[p]), b["T"][p]) for p in ref]
    cfg, sd, imgs, points, b = W.tower("clip")
    for r in range(W.B):
        ref, got = points(cfg, sd, imgs[r:r + 1]), W.clip_storage(cfg, sd, imgs[r:r + 1])
        single += [("clip image %d" % r, p, W.e(got[p], ref[p]), b["T"][p]) for p in ref]
    lines += ["%-18s %-5s model %.3e  T_p %.3e" % s for s in single]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for name, b in tables:
        for p, t in b["T"].items():
            d1, d2 = b["draws"][0][p], b["draws"][1][p]
            assert d1 <= t / 2 and d2 <= t / 2 and t == 2 * max(d1, d2)
            if name.startswith("t5") and p == "x0":
                assert t == 0                    # a gather from a bf16 table
                continue
            assert 0.8 <= d1 / d2 <= 1.25, (name, p, d1, d2)
            assert 1e-3 < t < 4e-2, (name, p, t)  # a few bf16 roundings of values of order one; far from the old 3e-2 per ELEMENT
    assert all(m <= t for _, _, m, t in single), [s for s in single if not s[2] <= s[3]]


def test_b_every_catalogue_entry_is_visible_or_exempt_with_its_proof(capsys):
    rows = {t: W.visibility(t) for t in ("t5", "clip", "pre")}
    with capsys.disabled():
        print("\n%-78s %-5s %s" % ("catalogue entry", "point", "e / T_p"))
        for t in rows:
            for name, p, ratio, es in rows[t]:
                note = "   (exempt: %s)" % W.EXEMPT[name] if name in W.EXEMPT else ""
                print("%-78s %-5s %9.1f%s" % (name, p, ratio, note) if t != "pre" else "%-78s %-5s e = %.2e" % (name, p, es[p]))
    assert sum(len(r) for r in rows.values()) == len(W.CATALOGUE) and len(rows["t5"]) >= 28 and len(rows["clip"]) >= 37 and len(rows["pre"]) == 4
    assert set(W.EXEMPT) <= {c.name for c in W.CATALOGUE}
    # nothing but the two cases: the k third of to_qkv.bias (one entry per evaluated block) and tanh- against erf-GELU (one per tower)
    assert all(("to_qkv (k third)" in n and v == "cancels") or ("GELU" in n and "tanh" in n and v == "below T_p") for n, v in W.EXEMPT.items())
    assert len(W.EXEMPT) == 4
    for t in ("t5", "clip"):
        Tp = W.tower(t)[4]["T"]
        weak = [(n, p, r) for n, p, r, _ in rows[t] if r < 4.0 and n not in W.EXEMPT]
        assert not weak, weak
        for n, _, _, es in rows[t]:
            if W.EXEMPT.get(n) == "cancels":
                assert all(v <= 1e-5 for v in es.values()), (n, es)
            elif W.EXEMPT.get(n) == "below T_p":
                assert all(es[p] < Tp[p] for p in es if Tp[p]) and max(es.values()) > 0, (n, es)
    assert all(es["pre"] > 0.1 for _, _, _, es in rows["pre"])          # against a bound of a few 1e-6 (test_enc_wiring_gpu.py)


def test_catalogue_leaves_the_oracle_as_it_found_it():
    before = {(m.__name__, k): getattr(m, k) for m in (E, W) for k in dir(m)}
    for t in ("t5", "clip", "pre"):
        cfg, sd = (W.tower(t)[:2] if t != "pre" else ({}, {}))
        keys = {k: v.clone() for k, v in sd.items()}
        cfg0 = dict(cfg)
        for c in (c for c in W.CATALOGUE if c.tower == t):
            with W.applied(c, cfg, sd) as (cfg_m, sd_m):
                changed = cfg_m != cfg or any(getattr(m, k) is not v for m in (E, W) for (mn, k), v in before.items() if mn == m.__name__) \
                    or any(sd_m[k] is not sd[k] and not torch.equal(sd_m[k], sd[k]) for k in sd)
                assert changed, c.name
            assert all(getattr(m, k) is v for m in (E, W) for (mn, k), v in before.items() if mn == m.__name__), c.name
        assert cfg == cfg0 and all(torch.equal(sd[k], keys[k]) for k in sd)


# (c): entries that pass the old check.  The first group are no-ops on encoders_tiny.npz; the second change the output and still pass.
OLD_T5_NOOPS = [f"t5: gamma {k} replaced by 1" for k in W.T5_GAMMAS] + [f"t5: norm1 <-> norm2 gammas, layer {i}" for i in (0, 1)]
OLD_T5_PASS = ["t5: erf-GELU for tanh-GELU"]
OLD_VIT_NOOPS = [f"clip: LayerNorm weight {k} replaced by 1" for k in W.CLIP_NORMS] + [f"clip: LayerNorm bias {k} zeroed" for k in W.CLIP_NORMS] \
    + [f"clip: norm1 <-> norm2, block {i}" for i in (0, 1)]
OLD_VIT_PASS = ["clip: quick-GELU for GELU", "clip: tanh-GELU for erf-GELU", "clip: norm_eps 1e-6 for 1e-5"]


def test_c_the_old_check_passes_these_mutants(golden_dir, capsys):
    g = _golden(golden_dir, "encoders_tiny.npz")
    split = lambda prefix: {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    t5cfg = dict(num_heads=2, num_layers=2, num_buckets=32)
    vcfg = dict(num_heads=2, num_layers=3, patch_size=14, norm_eps=1e-5)
    lines = []
    for cfg, sd, run, want, noops, passing in (
            (t5cfg, split("t5."), lambda c, s: W.t5_points(c, s, dict(ids=g["ids"], mask=g["mask"]))["out"], g["t5_out"], OLD_T5_NOOPS, OLD_T5_PASS),
            (vcfg, split("vit."), lambda c, s: W.clip_points(c, s, g["imgs"])["out"], g["vit_out"], OLD_VIT_NOOPS, OLD_VIT_PASS)):
        ref = run(cfg, sd)
        torch.testing.assert_close(ref, want, rtol=1e-4, atol=1e-4)
        for name in noops + passing:
            with W.applied(W.by_name(name), cfg, sd) as (cfg_m, sd_m):
                got = run(cfg_m, sd_m)
            d = float((got - ref).abs().max())
            lines.append("%-62s max |d| %.1e" % (name, d))
            assert (d == 0) if name in noops else (d > 1e-6), (name, d)          # a no-op on this data / a real change ...
            assert torch.allclose(got, want, rtol=3e-2, atol=3e-2), name          # ... that the old tolerance does not see
    assert len(lines) == 7 + 1 + 12 + 3
    with capsys.disabled():
        print("\non encoders_tiny.npz, mutant against the unmutated fp32 oracle (each passes rtol = atol = 3e-2 against the golden):")
        print("\n".join(lines))


def test_oracle_matches_the_reference_on_the_planted_towers(golden_dir):
    g = _golden(golden_dir, "encoders_planted.npz")
    assert int(g["seed"]) == W.SEED
    inp, imgs, clip = W.planted_t5_inputs(), W.planted_images(), W.planted_clip()
    assert torch.equal(g["ids"], inp["ids"]) and torch.equal(g["mask"], inp["mask"]) and torch.equal(g["imgs"], imgs) and torch.equal(g["clip"], clip)
    cfg = W.T5CFG
    out = E.t5_encoder(W.planted_t5(), inp["ids"], inp["mask"], cfg["num_heads"], cfg["num_layers"], cfg["num_buckets"])
    torch.testing.assert_close(out, g["t5_out"], rtol=1e-4, atol=1e-4)
    cfg = W.VITCFG
    out = E.clip_visual_31(W.planted_vit(), imgs, cfg["num_heads"], cfg["num_layers"], cfg["patch_size"], cfg["norm_eps"])
    torch.testing.assert_close(out, g["vit_out"], rtol=1e-4, atol=1e-4)
    pre = W.pre_points(clip)["pre"]
    assert pre.shape == g["pre"].shape == (1, 3, 70, 70)
    torch.testing.assert_close(pre, g["pre"], rtol=1e-4, atol=1e-4)
