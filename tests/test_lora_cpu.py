"""LoRA adapters without a GPU (scail_amd/lora.py; include/scail_hip.h scail_lora_merge_bf16 / scail_add_scaled_bf16): the ABI and the
host-side refusals of the two entries, the planner on a fake network, the file readers, the CLI option, and the CPU restatement
(tests/lora_ref.py) against fp64."""
import ctypes
import math
import os
import re

import pytest
import torch

import lora_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, bf16 = torch.float32, torch.bfloat16
A = 0x1000          # a fake device address: validation fails, or the problem is empty, before it is ever dereferenced


@pytest.fixture(scope="module")
def lib():
    from scail_amd import build, lib as L
    build.build(verbose=False)
    return L.load()


def test_symbols_exported_declared_and_bound(lib):
    from scail_amd import lib as L, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scail_hip.h")).read(), flags=re.S)
    for name, nargs in (("scail_lora_merge_bf16", 11), ("scail_add_scaled_bf16", 8)):
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(L.SIGNATURES[name])
    assert callable(ops.lora_merge_) and callable(ops.add_scaled_)


def test_host_side_refusals(lib):
    from scail_amd import lib as L
    inf, nan = float("inf"), float("nan")
    m, a = "scail_lora_merge_bf16", "scail_add_scaled_bf16"
    cases = [
        (r"scail_lora_merge_bf16: N must be >= 0, got -1", m, (A, 8, -1, 8, A, 4, A, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: K must be >= 0, got -3", m, (A, 8, 2, -3, A, 4, A, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: r must be >= 0, got -2", m, (A, 8, 2, 8, A, 4, A, 8, -2, 1.0, None)),
        (r"scail_lora_merge_bf16: r must be below 2\^15 = 32768, got 32768", m, (A, 8, 2, 8, A, 32768, A, 8, 32768, 1.0, None)),
        (r"scail_lora_merge_bf16: ldw = 7 is smaller than K = 8", m, (A, 7, 2, 8, A, 4, A, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: ld_up = 3 is smaller than r = 4", m, (A, 8, 2, 8, A, 3, A, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: ld_down = 5 is smaller than K = 8", m, (A, 8, 2, 8, A, 4, A, 5, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: scale must be finite, got -?nan", m, (A, 8, 2, 8, A, 4, A, 8, 4, nan, None)),
        (r"scail_lora_merge_bf16: scale must be finite, got inf", m, (A, 8, 2, 8, A, 4, A, 8, 4, inf, None)),
        (r"scail_lora_merge_bf16: null pointer: w \(N = 2, K = 8, r = 4\)", m, (None, 8, 2, 8, A, 4, A, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: null pointer: up", m, (A, 8, 2, 8, None, 4, A, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: null pointer: down", m, (A, 8, 2, 8, A, 4, None, 8, 4, 1.0, None)),
        (r"scail_lora_merge_bf16: the grid must stay below 2\^31 workgroups, got 1073741824 x 2 tiles", m,
         (A, 256, 1 << 36, 256, A, 4, A, 256, 4, 1.0, None)),
        (r"scail_add_scaled_bf16: N must be >= 0, got -1", a, (A, 8, -1, 8, A, 8, 1.0, None)),
        (r"scail_add_scaled_bf16: K must be >= 0, got -8", a, (A, 8, 1, -8, A, 8, 1.0, None)),
        (r"scail_add_scaled_bf16: ldw = 7 is smaller than K = 8", a, (A, 7, 2, 8, A, 8, 1.0, None)),
        (r"scail_add_scaled_bf16: ldd = 6 is smaller than K = 8", a, (A, 8, 2, 8, A, 6, 1.0, None)),
        (r"scail_add_scaled_bf16: scale must be finite, got -inf", a, (A, 8, 2, 8, A, 8, -inf, None)),
        (r"scail_add_scaled_bf16: null pointer: w \(N = 2, K = 8\)", a, (None, 8, 2, 8, A, 8, 1.0, None)),
        (r"scail_add_scaled_bf16: null pointer: d", a, (A, 8, 2, 8, None, 8, 1.0, None)),
        (r"scail_add_scaled_bf16: the grid must stay below 2\^31 workgroups, got N = 1099511627776 rows of 1 8-column groups", a,
         (A, 8, 1 << 40, 8, A, 8, 1.0, None)),
    ]
    for needle, name, args in cases:
        with pytest.raises(L.ScailHipError, match=needle):
            L.call(name, *args)
    # empty problems launch nothing and need no device, whatever the pointers
    L.call(m, None, 8, 0, 8, None, 4, None, 8, 4, 1.0, None)
    L.call(m, None, 8, 2, 0, None, 4, None, 8, 4, 1.0, None)
    L.call(m, None, 8, 2, 8, None, 0, None, 8, 0, 1.0, None)
    L.call(a, None, 8, 0, 8, None, 8, 1.0, None)
    L.call(a, None, 8, 2, 0, None, 8, 1.0, None)


# ---- the planner on a fake network ------------------------------------------------------------------------------------------------------------
class FakeNet:
    """param_spec() of a 2-layer D = 128 network and nothing else: every other access is recorded (a refused adapter must make none)"""
    hidden_size, inner_hidden_size, time_embed_dim, time_freq_dim, text_dim, clip_dim, num_layers = 128, 256, 128, 64, 64, 1280, 2

    def __init__(self):
        self.calls = []
        self.loras = []

    def param_spec(self):
        from scail_amd.dit import DiffusionTransformer
        return DiffusionTransformer.param_spec(self)

    def named_parameters(self):
        self.calls.append("named_parameters")
        return iter(())

    def weights_changed(self):
        self.calls.append("weights_changed")


D = FakeNet.hidden_size


def _pair(n, k, r, seed, dtype=f32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, r, generator=g).to(dtype), torch.randn(r, k, generator=g).to(dtype)


def _strip(plan):
    return [(e.param, e.row_offset, e.rows, e.kind, e.scale, e.rank, e.alpha) for e in plan]


def _same_plan(a, b):
    assert _strip(a) == _strip(b)
    for x, y in zip(a, b):
        assert (x.up is None) == (y.up is None) and (x.up is None or torch.equal(x.up, y.up)) and torch.equal(x.down, y.down)


def test_plan_conventions_agree():
    from scail_amd import lora
    net = FakeNet()
    upq, dnq = _pair(D, D, 4, 1)
    upk, dnk = _pair(D, D, 4, 2)
    upv, dnv = _pair(D, D, 4, 3)
    upo, dno = _pair(D, D, 2, 4)
    wan = {"diffusion_model.blocks.1.self_attn.q.lora_A.weight": dnq, "diffusion_model.blocks.1.self_attn.q.lora_B.weight": upq,
           "blocks.1.self_attn.k.lora_down.weight": dnk, "blocks.1.self_attn.k.lora_up.weight": upk,
           "blocks.1.self_attn.v.lora_A.weight": dnv, "blocks.1.self_attn.v.lora_B.weight": upv,
           "blocks.1.self_attn.o.lora_A.weight": dno, "blocks.1.self_attn.o.lora_B.weight": upo, "blocks.1.self_attn.o.alpha": torch.tensor(3.0),
           "blocks.1.norm3.diff": torch.ones(D), "blocks.1.norm3.diff_b": torch.ones(D), "blocks.1.modulation.diff": torch.ones(1, 6, D)}
    plan = lora.plan_adapter(net, wan, 0.5)
    qkv = "transformer.layers.1.attention.query_key_value.weight"
    assert _strip(plan)[:2] == [("mixins.adaln_layer.adaLN_modulations.1", 0, 1, "diff", 0.5, 0, None),
                                (qkv, 0, D, "lora", 0.5, 4, 4.0)]
    assert [(e.param, e.row_offset) for e in plan if e.param == qkv] == [(qkv, 0), (qkv, D), (qkv, 2 * D)]
    o = next(e for e in plan if e.param.endswith("attention.dense.weight"))
    assert (o.rank, o.alpha, o.scale) == (2, 3.0, 0.75)
    # the other suffix spelling, without the prefix
    other = {}
    for k, v in wan.items():
        k = k.replace("diffusion_model.", "")
        k = (k.replace("lora_A", "lora_down").replace("lora_B", "lora_up") if "lora_A" in k or "lora_B" in k
             else k.replace("lora_down", "lora_A").replace("lora_up", "lora_B"))
        other[k] = v
    _same_plan(plan, lora.plan_adapter(net, other, 0.5))
    # native names: the o, norm and table entries under the SAT names; q / k / v have no native name of their own (the fused matrix is one)
    native = {"transformer.layers.1.attention.dense.lora_A.weight": dno, "transformer.layers.1.attention.dense.lora_B.weight": upo,
              "transformer.layers.1.attention.dense.alpha": torch.tensor(3.0),
              "transformer.layers.1.post_cross_attention_layernorm.diff": torch.ones(D),
              "transformer.layers.1.post_cross_attention_layernorm.diff_b": torch.ones(D),
              "mixins.adaln_layer.adaLN_modulations.1.diff": torch.ones(1, 6, D)}
    sub = {k: v for k, v in wan.items() if ".self_attn.o." in k or "norm3" in k or "modulation" in k}
    _same_plan(lora.plan_adapter(net, sub, 0.5), lora.plan_adapter(net, native, 0.5))
    # the whole fused matrix and the patch embedding as (D, 80) under their native names
    up3, dn3 = _pair(3 * D, D, 3, 5)
    upp, dnp = _pair(D, 80, 2, 6)
    p = lora.plan_adapter(net, {"transformer.layers.0.attention.query_key_value.lora_A.weight": dn3,
                                "transformer.layers.0.attention.query_key_value.lora_B.weight": up3,
                                "mixins.patch_embed.proj.lora_A.weight": dnp, "mixins.patch_embed.proj.lora_B.weight": upp})
    assert _strip(p) == [("mixins.patch_embed.proj.weight", 0, D, "lora", 1.0, 2, 2.0),
                         ("transformer.layers.0.attention.query_key_value.weight", 0, 3 * D, "lora", 1.0, 3, 3.0)]
    assert net.calls == []


def test_plan_scale_is_rounded_once():
    from scail_amd import lora
    net = FakeNet()
    t = {"blocks.0.ffn.0.lora_A.weight": _pair(256, D, 7, 8)[1], "blocks.0.ffn.0.lora_B.weight": _pair(256, D, 7, 8)[0]}
    assert lora.plan_adapter(net, t)[0].scale == 1.0 and lora.plan_adapter(net, t)[0].alpha == 7.0          # a missing alpha is the rank
    t["blocks.0.ffn.0.alpha"] = torch.tensor([0.3], dtype=torch.float16)
    alpha = float(torch.tensor(0.3, dtype=torch.float16))
    for strength in (1.0, 0.1, -2.7, 1e-3):
        e = lora.plan_adapter(net, t, strength)[0]
        want = float(torch.tensor(strength * alpha / 7, dtype=torch.float64).to(f32))
        assert e.scale == want == R.scale_of(strength, alpha, 7) and e.alpha == alpha
        assert e.scale != strength * alpha / 7 or strength * alpha / 7 == want        # fp32, not the Python double
    d = lora.plan_adapter(net, {"blocks.0.ffn.0.diff": torch.zeros(256, D, dtype=bf16)}, 0.1)[0]
    assert d.scale == float(torch.tensor(0.1, dtype=f32)) and d.kind == "diff" and d.rank == 0 and d.alpha is None


def test_every_alias_resolves_to_a_slice_of_a_parameter():
    from scail_amd import lora
    net = FakeNet()
    spec = net.param_spec()
    al = lora.wan_aliases(net)
    assert len(al) == net.num_layers * 19 + 11
    for name, t in al.items():
        assert lora.resolve(name, spec, al) == t
        assert t.weight in spec, name
        assert t.bias is None or t.bias in spec, name
        rows = spec[t.weight][0] if t.rows is None else t.rows
        assert 0 <= t.row_offset and rows > 0 and t.row_offset + rows <= spec[t.weight][0], name
        if t.bias is not None:
            assert t.row_offset + rows <= spec[t.bias][0], name


def test_aliases_of_a_block_cover_its_matrices_exactly_once():
    from scail_amd import lora
    net = FakeNet()
    spec = net.param_spec()
    al = lora.wan_aliases(net)
    for i in range(net.num_layers):
        mats = {n: s for n, s in spec.items() if len(s) == 2 and (n.startswith(f"transformer.layers.{i}.") or
                                                                  n == f"mixins.adaln_layer.clip_feature_key_value_list.{i}.weight")}
        assert len(mats) == 8
        cover = {n: torch.zeros(s[0], dtype=torch.int32) for n, s in mats.items()}
        for name, t in al.items():
            if name.startswith(f"blocks.{i}.") and t.weight in cover:
                rows = spec[t.weight][0] if t.rows is None else t.rows
                cover[t.weight][t.row_offset:t.row_offset + rows] += 1
        for n, c in cover.items():
            assert bool((c == 1).all()), n


def _good():
    up, dn = _pair(D, D, 4, 11)
    return {"blocks.0.self_attn.q.lora_A.weight": dn, "blocks.0.self_attn.q.lora_B.weight": up}


REFUSALS = {
    "no parameter": ({"blocks.9.self_attn.q.lora_A.weight": torch.zeros(4, D)}, 1.0, r"blocks\.9\.self_attn\.q\.lora_A\.weight.*resolves to no parameter"),
    "unknown module": ({"blocks.0.self_attn.w.diff": torch.zeros(D, D)}, 1.0, r"blocks\.0\.self_attn\.w\.diff.*resolves to no parameter"),
    "not an adapter key": ({"blocks.0.self_attn.q.weight": torch.zeros(D, D)}, 1.0, r"blocks\.0\.self_attn\.q\.weight: not an adapter key"),
    "half a pair (down)": ({"blocks.0.self_attn.q.lora_A.weight": torch.zeros(4, D)}, 1.0, r"blocks\.0\.self_attn\.q\.lora_A\.weight: a pair with only one half"),
    "half a pair (up)": ({"blocks.0.self_attn.q.lora_up.weight": torch.zeros(D, 4)}, 1.0, r"blocks\.0\.self_attn\.q\.lora_up\.weight: a pair with only one half"),
    "ranks differ": ({"blocks.0.self_attn.q.lora_A.weight": torch.zeros(4, D), "blocks.0.self_attn.q.lora_B.weight": torch.zeros(D, 5)}, 1.0,
                     r"blocks\.0\.self_attn\.q\.lora_B\.weight: ranks differ"),
    "up rows": ({"blocks.0.self_attn.q.lora_A.weight": torch.zeros(4, D), "blocks.0.self_attn.q.lora_B.weight": torch.zeros(3 * D, 4)}, 1.0,
                r"blocks\.0\.self_attn\.q\.lora_B\.weight: up \(384, 4\) does not match the slice: 128 rows"),
    "down columns": ({"blocks.0.ffn.2.lora_A.weight": torch.zeros(4, D), "blocks.0.ffn.2.lora_B.weight": torch.zeros(D, 4)}, 1.0,
                     r"blocks\.0\.ffn\.2\.lora_A\.weight: down \(4, 128\) does not match the slice: 256 columns"),
    "pair on a norm": ({"blocks.0.norm3.lora_A.weight": torch.zeros(1, D), "blocks.0.norm3.lora_B.weight": torch.zeros(D, 1)}, 1.0,
                       r"blocks\.0\.norm3\.lora_A\.weight.*resolves to no parameter that takes a low-rank pair"),
    "diff shape": ({"blocks.0.self_attn.k.diff": torch.zeros(3 * D, D)}, 1.0, r"blocks\.0\.self_attn\.k\.diff: a difference of shape \(384, 128\) for \(128, 128\)"),
    "diff_b shape": ({"blocks.0.ffn.0.diff_b": torch.zeros(D)}, 1.0, r"blocks\.0\.ffn\.0\.diff_b: a difference of shape \(128,\) for \(256,\)"),
    "diff_b without bias": ({"blocks.0.modulation.diff_b": torch.zeros(D)}, 1.0, r"blocks\.0\.modulation\.diff_b.*no parameter with a bias"),
    "alpha nan": (dict(_good(), **{"blocks.0.self_attn.q.alpha": torch.tensor(float("nan"))}), 1.0, r"blocks\.0\.self_attn\.q\.alpha: alpha must be a finite scalar"),
    "alpha inf": (dict(_good(), **{"blocks.0.self_attn.q.alpha": torch.tensor(float("inf"))}), 1.0, r"blocks\.0\.self_attn\.q\.alpha: alpha must be a finite scalar"),
    "alpha vector": (dict(_good(), **{"blocks.0.self_attn.q.alpha": torch.ones(2)}), 1.0, r"blocks\.0\.self_attn\.q\.alpha: alpha must be a finite scalar"),
    "alpha alone": ({"blocks.0.self_attn.q.alpha": torch.tensor(1.0)}, 1.0, r"blocks\.0\.self_attn\.q\.alpha: an alpha without a pair"),
    "integer tensor": (dict(_good(), **{"blocks.0.self_attn.o.diff": torch.zeros(D, D, dtype=torch.int32)}), 1.0,
                       r"blocks\.0\.self_attn\.o\.diff: expected a floating-point tensor, got torch\.int32"),
    "strength nan": (_good(), float("nan"), r"strength must be finite, got nan"),
    "strength inf": (_good(), float("inf"), r"strength must be finite, got inf"),
    "empty": ({}, 1.0, r"the adapter yields no entry"),
    "one module twice": (dict(_good(), **{"transformer.layers.0.attention.query_key_value.lora_A.weight": torch.zeros(2, D),
                                          "transformer.layers.0.attention.query_key_value.lora_B.weight": torch.zeros(3 * D, 2)}), 1.0,
                         r"targets the same rows of transformer\.layers\.0\.attention\.query_key_value\.weight"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_plan_refusals_name_the_key_and_touch_nothing(name):
    from scail_amd import lora
    from scail_amd.dit import DiffusionTransformer
    tensors, strength, needle = REFUSALS[name]
    net = FakeNet()
    with pytest.raises(ValueError, match=needle):
        lora.plan_adapter(net, tensors, strength)
    # the public entry on the recording network: refused before a single parameter was asked for
    with pytest.raises(ValueError, match=needle):
        DiffusionTransformer.merge_lora(net, tensors, strength)
    assert net.calls == [] and net.loras == []


def test_merge_refuses_meta_and_host_parameters_by_name():
    from scail_amd import lib as L
    from scail_amd.dit import DiffusionTransformer
    kw = dict(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
              time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True, use_i2v_clip=True)
    meta = DiffusionTransformer(init_seed=None, **kw)
    with pytest.raises(ValueError, match=r"transformer\.layers\.0\.attention\.query_key_value\.weight is a meta parameter"):
        meta.merge_lora(_good())
    host = DiffusionTransformer(device="cpu", **kw)
    before = {k: v.clone() for k, v in host.state_dict().items()}
    with pytest.raises(L.ScailHipError, match=r"transformer\.layers\.0\.attention\.query_key_value\.weight is on cpu.*GPU"):
        host.merge_lora(_good())
    assert all(torch.equal(v, host.state_dict()[k]) for k, v in before.items()) and host.loras == [] and meta.loras == []


def test_read_adapter_round_trip(tmp_path):
    from safetensors.torch import save_file
    from scail_amd import lora
    up, dn = _pair(D, D, 4, 12, torch.float16)
    t = {"blocks.0.self_attn.q.lora_A.weight": dn, "blocks.0.self_attn.q.lora_B.weight": up, "blocks.0.self_attn.q.alpha": torch.tensor(2.0),
         "blocks.0.norm3.diff_b": torch.randn(D).to(bf16)}
    save_file(t, str(tmp_path / "a.safetensors"))
    torch.save(t, str(tmp_path / "a.pt"))
    torch.save({"state_dict": t}, str(tmp_path / "b.pt"))
    for f in ("a.safetensors", "a.pt", "b.pt"):
        got = lora.read_adapter(str(tmp_path / f))
        assert set(got) == set(t)
        for k in t:
            assert got[k].dtype == t[k].dtype and got[k].device.type == "cpu" and torch.equal(got[k], t[k]), (f, k)
        _same_plan(lora.plan_adapter(FakeNet(), got, 0.5), lora.plan_adapter(FakeNet(), t, 0.5))
    torch.save([1, 2], str(tmp_path / "c.pt"))
    with pytest.raises(ValueError, match="expected a dict of tensors"):
        lora.read_adapter(str(tmp_path / "c.pt"))


def test_cli_lora_option():
    from scail_amd import cli
    a = cli.build_parser().parse_args(["--tiny", "--lora", "a:0.5", "--lora", "b"])
    assert a.lora == ["a:0.5", "b"]
    assert [cli.lora_arg(v) for v in a.lora] == [("a", 0.5), ("b", 1.0)]
    assert cli.lora_arg("dir/x.safetensors:-1.25") == ("dir/x.safetensors", -1.25)
    assert cli.lora_arg("c:/x.pt") == ("c:/x.pt", 1.0)              # what follows the colon is no number: part of the path
    assert cli.build_parser().parse_args([]).lora == []
    with pytest.raises(ValueError, match="finite"):
        cli.lora_arg("a:nan")


@pytest.mark.parametrize("r", [1, 7, 64])
def test_restatement_is_inside_the_bound(r):
    """The torch expression of tests/lora_ref.py against the fp64 truth T = w + s * sum_j up_j down_j (u = 2^-24, gamma_n = n u / (1 - n u)):
      * each product p_j carries one rounding and the running sum r - 1 more (0 + p_0 is exact): |acc - sum_j p_j| <= gamma_r S,
        S = sum_j |up_j down_j|;
      * scale * acc is one more rounding: |sa - s sum_j p_j| <= gamma_{r+1} |s| S  (<= gamma_{r+2} |s| S, the bound used);
      * w + sa is rounded once in fp32: at most half an fp32 ulp of the sum (one ulp is allowed);
      * the sum is rounded once to bf16: at most half a bf16 ulp of the result.
    Magnitudes: N(0, 1) factors and weights with |w| >= 2^-6, s = 0.37: nothing overflows or leaves the normal range, the fp64
    evaluation's own error (2^-53 relative) is far below every term."""
    g = torch.Generator().manual_seed(100 + r)
    N, K, s = 48, 40, 0.37
    up, down = torch.randn(N, r, generator=g), torch.randn(r, K, generator=g)
    w = torch.randn(N, K, generator=g)
    w = (torch.sign(w) * w.abs().clamp_min(2.0 ** -6)).to(bf16)
    scale = R.scale_of(s, r, r)
    got = R.cpu_merge(w, up, down, scale).double()
    prods = up.double().unsqueeze(2) * down.double().unsqueeze(0)                    # (N, r, K), exact in fp64
    truth = w.double() + scale * prods.sum(1)
    S = prods.abs().sum(1)
    sum32 = (w.float() + torch.tensor(scale, dtype=f32) * R.cpu_acc(up, down)).double()
    ulp32 = torch.exp2(torch.floor(torch.log2(sum32.abs())) - 23.0)
    bound = 0.5 * R.bf16_ulp(got) + R.gamma(r + 2) * abs(scale) * S + ulp32
    assert bool(torch.isfinite(got).all()) and bool((got != 0).all())
    err = (got - truth).abs()
    assert bool((err <= bound).all()), f"r {r}: worst error / bound {float((err / bound).max())}"
    assert float((err / bound).max()) > 0.5                                     # the bound is not loose: the bf16 rounding dominates it
