"""The SAT seam on the host side, without a GPU: scail_amd.sat_mixins hooks ``layer_forward`` (seam B2) / ``attention_fn``
(seam B3) into the reference ``DiffusionTransformer`` through ``add_mixin`` (sat/model/base_model.py:114-176).  Checked here:
engine_from_reference over a network with the reference's attributes and state-dict layout, the hooks refuse a
sequence-parallel SAT world, and HipBackend.block's per-forward conditioning cache.  The GPU side of the
contract (the same calls through HipBackend, against the reference's golden output) is tests/test_sat_mixins_gpu.py."""
import pytest
import torch


class _ReferenceNetStandIn(torch.nn.Module):
    """What engine_from_reference reads from a live reference DiffusionTransformer (dit...:1209-1321): its constructor hyper-parameters
    as attributes and its parameters under the reference state-dict layout (oracle.state_dict_spec, pinned by test_abi)."""

    def __init__(self, cfg, sd):
        super().__init__()
        from scail_amd.dit import _register
        for k in ("num_frames", "time_compressed_rate", "latent_width", "latent_height", "in_channels", "out_channels", "hidden_size",
                  "text_dim", "num_layers", "num_attention_heads", "time_freq_dim", "time_embed_dim", "inner_hidden_size",
                  "layernorm_epsilon"):
            setattr(self, k, getattr(cfg, k))
        self.patch_size, self.share_adaln, self.use_i2v_clip = list(cfg.patch_size), True, True
        for name, t in sd.items():
            _register(self, name, torch.nn.Parameter(t, requires_grad=False))


def test_engine_from_reference_shares_the_reference_parameters():
    """engine_from_reference(): strict state-dict match, parameters attached by reference (no copy)."""
    from oracle import scail_oracle as O
    from scail_amd import sat_mixins
    cfg = O.DiTConfig(**O.TINY)
    sd = O.make_state_dict(cfg, seed=3)
    net = _ReferenceNetStandIn(cfg, sd)
    assert set(net.state_dict()) == set(O.state_dict_spec(cfg))
    eng = sat_mixins.engine_from_reference(net)
    a = dict(net.named_parameters())["transformer.layers.1.mlp.dense_h_to_4h.weight"]
    b = dict(eng.named_parameters())["transformer.layers.1.mlp.dense_h_to_4h.weight"]
    assert a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape)
    assert set(dict(eng.named_parameters())) == set(net.state_dict())
    with pytest.raises(TypeError):
        sat_mixins.install(torch.nn.Linear(2, 2))


def test_hooks_refuse_a_sequence_parallel_world(monkeypatch):
    """both seams replace code that exchanges between sequence-parallel ranks (UlyessAttentionMixin.attention_fn,
    dit...:351-379); with SAT's sequence-parallel world > 1 they must raise instead of attending to the local shard only."""
    import sys
    import types
    from scail_amd import sat_mixins
    from scail_amd import lib as L
    stub = types.ModuleType("sat.mpu")
    stub.get_sequence_parallel_world_size = lambda: 2
    monkeypatch.setitem(sys.modules, "sat.mpu", stub)
    assert sat_mixins._sequence_parallel_world_size() == 2
    q = torch.zeros(1, 2, 8, 128, dtype=torch.bfloat16)
    with pytest.raises(L.ScailHipError, match="sequence-parallel world size is 2"):
        sat_mixins.HipAttentionMixin(backend=object())._hip_attention(q, q, q, None)
    with pytest.raises(L.ScailHipError, match="sequence-parallel world size is 2"):
        sat_mixins.HipLayerMixin(backend=object()).layer_forward(torch.zeros(1, 4, 8), None, layer_id=0)
    stub.get_sequence_parallel_world_size = lambda: 1
    assert sat_mixins._sequence_parallel_world_size() == 1

    def boom():
        raise AssertionError("sequence parallel group is not initialized")      # sat/mpu/initialize.py asserts when unset
    stub.get_sequence_parallel_world_size = boom
    assert sat_mixins._sequence_parallel_world_size() == 1


def test_block_backend_conditioning_cache_is_per_forward():
    """HipBackend.block caches the per-layer cross-attention K / V of ONE forward.  A new forward (layer 0) or new
    conditioning objects must re-project, also when a freed tensor's address and _version come back (the old key)."""
    from scail_amd import sat_mixins

    class Eng:
        def __init__(self):
            self.n = 0

        def kv_conditioning(self, text, clip):
            self.n += 1
            return {"tag": float(text.flatten()[0])}

        def prepare(self):
            return {}

        def _rope(self, *a):
            return None, None

    class Step:
        def block(self, layer, hidden, mod, cond, cos, sin):
            return cond["tag"]

    be = sat_mixins.HipBackend(Eng())
    be._cstep = Step()
    h = torch.zeros(1, 2, 4)
    t1, c1 = torch.full((1, 2, 4), 1.0), torch.zeros(1, 2, 4)
    assert [be.block(i, h, None, t1, c1, (1, 1, 1, 0, 0)) for i in range(3)] == [1.0, 1.0, 1.0] and be.engine.n == 1
    assert be.block(0, h, None, t1, c1, (1, 1, 1, 0, 0)) == 1.0 and be.engine.n == 2          # next forward: layer 0 re-projects
    t2 = torch.full((1, 2, 4), 2.0)                                                            # another prompt mid-stack
    assert be.block(1, h, None, t2, c1, (1, 1, 1, 0, 0)) == 2.0 and be.engine.n == 3
    # dtype-converted copies per layer, keyed on the host's own objects: no re-projection inside one forward
    assert be.block(2, h, None, t2.clone(), c1.clone(), (1, 1, 1, 0, 0), cond_key=(t2, c1)) == 2.0 and be.engine.n == 3
    t2.add_(1.0)                                                                               # in-place edit bumps _version
    assert be.block(3, h, None, t2, c1, (1, 1, 1, 0, 0)) == 3.0 and be.engine.n == 4
