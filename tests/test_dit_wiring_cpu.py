"""The wiring net, proven on the CPU before anything runs on a GPU (helper and definitions: tests/dit_wiring.py).

N_p is the distance e(model, oracle) = ||a - b||_2 / ||b||_2 of the bf16-storage model from the fp32 oracle at observation point p (the
larger of two draws of the inputs); T_p = 2 N_p is the bound tests/test_dit_wiring_gpu.py holds every route of the HIP path to.

  (a) the model is within T_p / 2 on both draws, and the two draws agree to 25 % -- the metric is a root mean square over >= 29 000
      elements, so what differs between draws is the activation statistics, not sampling error; T_p does not rest on one draw.
  (b) every entry of the mutation catalogue moves the fp32 oracle by >= 4 T_p (8 x the modelled noise) at one observation point or more.
      The table (entry, best point, ratio to T_p) is printed.  NOT_VISIBLE (at most 4 entries, each with its reason and the kernel-level
      exact test that covers it) is empty: no entry needed the exemption.
  (c) for the record, the reason these tests exist: under oracle.make_state_dict and the dit_tiny inputs twelve mutants (the ten rows of
      the table in the issue that asked for this net; the last row is three gammas) pass the older tests' rtol = atol = 2e-2 at every
      hidden state and at the output, in fp32, with no bf16 noise at all.  If the old goldens are ever made discriminating, (c) is the
      test to delete.

Deliberately NOT in the catalogue: arithmetic-level changes -- eps 1e-6 against 1e-5, tanh against erf GELU, a 1 % softmax scale.  They sit
below the bf16 storage noise at any network-level point and belong to the kernel-level exact tests (tests/test_row_exact_*.py,
tests/test_gemm_exact_*.py, tests/test_attn_exact_*.py), which cover them.  A global RoPE shift of every token is not in it either: attention
sees position differences only, so it is an invariance, not an error."""
import os

import numpy as np
import pytest
import torch

import dit_wiring as DW
from oracle import scail_oracle as O


@pytest.fixture(scope="module")
def planted():
    cfg = DW.planted_config()
    return cfg, DW.planted_state_dict(cfg), DW.planted_inputs()


def test_planted_shapes(planted):
    cfg, sd, inp = planted
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.inner_hidden_size, cfg.num_layers) == (256, 2, 512, 2)
    pts = DW.oracle_points(cfg, sd, inp)
    assert pts["emb"].shape == (2, 96 + 288 + 72, 256) and 456 == 7 * 64 + 8 and pts["out"].shape == (2, 3, 16, 16, 24)
    assert inp["ctx"].shape == (2, 20, 64) and inp["clip"].shape == (1, 9, 1280)
    rows = inp["ctx"].reshape(40, 64)
    assert torch.unique(rows, dim=0).shape[0] == 40 and float(rows.abs().amax(1).min()) > 0          # distinct, none zero
    assert torch.equal(inp["x"][0], inp["x"][1]) and not torch.equal(inp["ctx"][0], inp["ctx"][1])
    for t in list(sd.values()) + [v for k, v in inp.items() if k != "t"]:
        assert torch.equal(t, DW.bf16r(t))                                                           # bf16-exact
    assert set(sd) == set(O.state_dict_spec(cfg)) and all(sd[k].shape == s for k, s in O.state_dict_spec(cfg).items())


def test_helper_restates_the_oracle(planted):
    """oracle_points is O.dit_forward bit for bit; the storage model without its roundings is the oracle up to fp32 re-association"""
    cfg, sd, inp = planted
    out, hidden = O.dit_forward(cfg, sd, inp["x"], inp["t"], inp["ctx"], inp["ref"], inp["pose"], inp["clip"], return_hidden=True)
    pts = DW.oracle_points(cfg, sd, inp)
    bi = DW.block_inputs_of(cfg, pts)
    pts = DW.oracle_points(cfg, sd, inp, bi)
    assert torch.equal(pts["out"], out) and all(torch.equal(pts[f"h{i}"], hidden[i]) for i in (1, 2)) and torch.equal(pts["emb"], hidden[0])
    ident = DW.storage_points(cfg, sd, inp, bi, r=lambda x: x)
    for p in DW.points_of(cfg):
        assert DW.e(ident[p], pts[p]) < 5e-6, p
    two = DW.planted_inputs(n_char=2)
    assert two["ref"].shape[1] == 2 and two["pose"].shape[1] == 6 and torch.equal(two["ref"][:, :1], inp["ref"])
    o2 = O.dit_forward(cfg, sd, two["x"], two["t"], two["ctx"], two["ref"], two["pose"], two["clip"])
    assert torch.equal(DW.oracle_points(cfg, sd, two)["out"], o2)


def test_a_noise_model_and_bounds(capsys):
    b = DW.bounds(sampler=True)
    with capsys.disabled():
        print("\npoint      N_p (draw 1)  N_p (draw 2)  T_p")
        for p in b["N"]:
            print("%-8s   %.3e     %.3e     %.3e" % (p, b["draws"][0][p], b["draws"][1][p], b["T"][p]))
    for p, t in b["T"].items():
        d1, d2 = b["draws"][0][p], b["draws"][1][p]
        assert d1 <= t / 2 and d2 <= t / 2 and t == 2 * max(d1, d2)
        assert 0.8 <= d1 / d2 <= 1.25, (p, d1, d2)
        assert 1e-3 < t < 4e-2, (p, t)           # a few bf16 roundings of values of order one; far from the old 2e-2 per ELEMENT
    two = DW.bounds(n_char=2)
    assert set(two["T"]) == set(DW.points_of(DW.planted_config()))


def test_b_every_catalogue_entry_is_visible(planted, capsys):
    cfg, sd, inp = planted
    rows = DW.visibility(cfg, sd, inp)
    with capsys.disabled():
        print("\n%-78s %-5s %s" % ("catalogue entry", "point", "e / T_p"))
        for name, p, ratio, _ in rows:
            print("%-78s %-5s %7.1f%s" % (name, p, ratio, "   (not visible: exempt)" if name in DW.NOT_VISIBLE else ""))
    assert len(rows) == len(DW.CATALOGUE) >= 60
    assert len(DW.NOT_VISIBLE) <= 4 and all(n in {c.name for c in DW.CATALOGUE} and len(v) == 2 for n, v in DW.NOT_VISIBLE.items())
    assert not set(DW.NOT_VISIBLE) & set(OLD_CHECK_MUTANTS)
    weak = [(n, p, r) for n, p, r, _ in rows if r < 4.0 and n not in DW.NOT_VISIBLE]
    assert not weak, weak
    # an exempt entry must really be invisible; a visible one has no business on the list
    assert all(r < 4.0 for n, _, r, _ in rows if n in DW.NOT_VISIBLE)


def test_catalogue_leaves_the_oracle_as_it_found_it(planted):
    cfg, sd, inp = planted
    before = {k: getattr(O, k) for k in dir(O)}
    keys = {k: v.clone() for k, v in sd.items()}
    for c in DW.CATALOGUE:
        with DW.applied(c, cfg, sd) as (cfg_m, sd_m):
            changed = cfg_m != cfg or any(getattr(O, k) is not v for k, v in before.items()) \
                or any(sd_m[k] is not sd[k] and not torch.equal(sd_m[k], sd[k]) for k in sd)
            assert changed, c.name
        assert all(getattr(O, k) is v for k, v in before.items()), c.name
    assert all(torch.equal(sd[k], keys[k]) for k in sd)


# the mutants of the first table of the issue, by their catalogue names
OLD_CHECK_MUTANTS = [
    "rope: global_rope_W -> 0", "rope: theta -> 9000",
    "bias dropped: query_key_value (v third), layer 1", "bias dropped: query_key_value (q third), layer 1",
    "bias dropped: attention dense, layer 1", "bias dropped: mlp dense_4h_to_h, layer 1",
    "bias dropped: post_cross_attention_layernorm, layer 1", "bias dropped: cross query, layer 1",
    "bias dropped: clip_feature_key_value (k half), layer 1",
    "gamma: query replaced by 1, layer 1", "gamma: key replaced by 1, layer 1", "gamma: cross_key replaced by 1, layer 1"]


def test_c_the_old_check_passes_these_mutants(golden_dir, capsys):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, "dit_tiny.npz")).items()}
    cfg = O.DiTConfig(**O.TINY)
    sd = O.make_state_dict(cfg, seed=int(g["seed"]))
    inp = dict(x=g["x"], t=g["t"], ctx=g["ctx"], ref=g["ref"], pose=g["pose"], clip=g["clip"])
    ref = DW.oracle_points(cfg, sd, inp)
    lines = []
    for name in OLD_CHECK_MUTANTS:
        with DW.applied(DW.by_name(name), cfg, sd) as (cfg_m, sd_m):
            got = DW.oracle_points(cfg_m, sd_m, inp)
        worst = max(float((got[p] - ref[p]).abs().max()) for p in ("h1", "h2", "out"))
        lines.append("%-62s max |d| %.1e  worst rel-L2 %.1e" % (name, worst, max(DW.e(got[p], ref[p]) for p in ("h1", "h2", "out"))))
        assert worst > 1e-4, name                                                       # the mutant does change the network ...
        for p in ("h1", "h2", "out"):                                                   # ... and the old tolerance does not see it
            assert torch.allclose(got[p], ref[p], rtol=2e-2, atol=2e-2), (name, p)
    with capsys.disabled():
        print("\nunder make_state_dict + dit_tiny, mutant against the unmutated fp32 oracle (passes rtol = atol = 2e-2):")
        print("\n".join(lines))
