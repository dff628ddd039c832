"""Every entry of the two C executors (csrc/dit_step.hip, csrc/vae_exec.hip) on a poisoned, guarded, exact-size workspace
(tests/ws_contract.py).

Each case runs one entry, through the project's own Python layers, once per fill (0x00, 0xFF = NaN in every element type, 0x47 = a large
finite number) on the same inputs, with the workspace and every buffer the bindings allocate handed out between guard bands at exactly the
queried size.  The outputs must be finite, bit-equal to each other and to one plain run on an ordinary workspace; the bands must be intact and
every input -- parameters, prepared weights, the fp8 weight buffer, conditioning, rope tables, x / ref / pose / latent -- must hold its bits.
No tolerance anywhere: every comparison is bit equality of the same computation.  A difference between fills is a dependence on memory the call
never wrote; a damaged band is a query that answers too little or a kernel that writes out of its buffer."""
import pytest
import torch

import conv_exact
import ws_contract as W

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOY = dict(hidden_size=512, num_attention_heads=4, inner_hidden_size=1024, text_dim=64, time_freq_dim=256, time_embed_dim=512)   # test_attn_vrows_gpu.TOY
TINY2 = dict(hidden_size=256, num_attention_heads=2, inner_hidden_size=512, text_dim=64, time_freq_dim=256, time_embed_dim=256)  # test_multichar_gpu.TINY2
LAYERS = 3                      # a first, a middle and the row-pruned last layer
SMALL = (3, 8, 20)              # T, H, W: Ltok 190 -- below one 256-row tile, one ragged 64-key tile
LARGE = (2, 28, 36)             # Ltok 882 -- 13 whole key tiles + 50 keys, above the 768-row boundary of the attention plan


def _ltok(T, H, W, n_char=1):
    return (n_char + T) * (H // 2) * (W // 2) + n_char * T * (H // 4) * (W // 4)


assert _ltok(*SMALL) == 190 and _ltok(*LARGE) == 882

_nets = {}


def _net(kind="toy", **kw):
    import test_parallel_gpu as P
    key = (kind,) + tuple(sorted(kw.items()))
    if key not in _nets:
        _nets[key] = P._mk(dict(TOY if kind == "toy" else TINY2, **kw), LAYERS, seed=77)
    return _nets[key]


def _inputs(shape, n_char=1, pair=False, seed=11):
    import test_parallel_gpu as P
    x, t, ctx, ref, pose, clip = P._inputs(*shape, n_char, 64, 12, 5, seed=seed)
    if pair:
        x = torch.cat([x[:1], x[:1]]).contiguous()
    return x, t, ctx, ref, pose, clip


def _fwd(net, inputs, **kw):
    x, t, ctx, ref, pose, clip = inputs
    return net.forward_f32(x, t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref,
                           concat_smpl_render=pose, **kw)


def _dit_objs(net, inputs, **more):
    """everything a DiT call reads and does not own: evaluated before AND after the plain run (the prepared weights, the conditioning and
    the executor exist after it)"""
    def objs():
        cs = getattr(net, "_cstep", None)
        return dict(net=net, prepared=getattr(net, "_prepared", None), fp8=getattr(cs, "_fp8_buf", None), cond=getattr(net, "_cond_cache", None),
                    rope=getattr(net, "_rope_cache", None), inputs=inputs, **more)
    return objs


def _as_list(r):
    return [t.clone() for t in (r if isinstance(r, (list, tuple)) else [r])]


def _contract(run, objs, expect_what=None):
    """The six steps of a case.  ``run() -> tensor(s)``; ``objs() -> dict`` of what must keep its bits.  -> the plain result(s)"""
    before = W.snapshot(objs())
    plain = _as_list(run())
    torch.cuda.synchronize()
    W.assert_unchanged(before)
    snap = W.snapshot(objs())
    got = {}
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got[name] = _as_list(run())
            s.check()                                                        # 5. the guards, around the workspace(s) and around the outputs
            if expect_what is not None:
                assert any(expect_what in what for what, _ in s.workspaces), [what for what, _ in s.workspaces]
    for name, outs in got.items():
        for o in outs:
            if o.dtype.is_floating_point:
                assert bool(torch.isfinite(o).all()), f"fill {name}: {int((~torch.isfinite(o)).sum())} non-finite output values"     # 2.
    for name, outs in got.items():
        for i, (o, z, p) in enumerate(zip(outs, got["zero"], plain)):
            assert o.shape == z.shape == p.shape
            assert torch.equal(o, z), f"output {i}: fill {name} differs from fill zero in {int((o != z).sum())} values"                 # 3.
            assert torch.equal(o, p), f"output {i}: fill {name} differs from the plain run in {int((o != p).sum())} values"           # 4.
    W.assert_unchanged(snap)                                                                                                          # 6.
    return plain


# ---- DiT: step ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vrows", [1, 0], ids=["vrows", "vt"])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["L190", "L882"])
def test_step(shape, vrows):
    """B 2; the V^T staging region is live only with attn_vrows 0"""
    net, inputs = _net(), _inputs(shape)
    out = conv_exact.with_options({"attn_vrows": vrows}, lambda: _contract(lambda: _fwd(net, inputs), _dit_objs(net, inputs)), {"attn_vrows": 1})[0]
    assert net._cstep is not None and out.shape == inputs[0].shape and not torch.equal(out[0], out[1])


def test_step_cfg_pair():
    """element 1 of hid is not filled in until block_tail's copy"""
    net, inputs = _net(), _inputs(SMALL, pair=True)
    out = _contract(lambda: _fwd(net, inputs, cfg_pair=True), _dit_objs(net, inputs))[0]
    assert torch.equal(out, _fwd(net, inputs)) and not torch.equal(out[0], out[1])


def test_step_two_characters():
    net, inputs = _net("tiny2"), _inputs(SMALL, n_char=2)
    assert inputs[3].shape[1] == 2 and inputs[4].shape[1] == 2 * SMALL[0]
    _contract(lambda: _fwd(net, inputs), _dit_objs(net, inputs), expect_what="chars_workspace_bytes")


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "cfg_pair"])
@pytest.mark.parametrize("scaling", ["row", "mx"])
def test_step_fp8(scaling, pair):
    """xq is sized for the widest K (the MLP's 1024): the 512-wide GEMMs leave stale codes behind their rows"""
    net, inputs = _net(gemm_precision="fp8", fp8_scaling=scaling), _inputs(SMALL, pair=pair)
    _contract(lambda: _fwd(net, inputs, cfg_pair=pair), _dit_objs(net, inputs))
    assert net._cstep._fp8_buf is not None and net._cstep.fp8_scaling == scaling


@pytest.mark.parametrize("scaling", ["row", "mx"])
def test_step_fp8_probe(scaling):
    """the probe's two result buffers come out of guarded_like under the same three fills (CStep.fp8_probe_on's torch.empty)"""
    net, inputs = _net(gemm_precision="fp8", fp8_scaling=scaling), _inputs(SMALL)
    x, t, ctx, ref, pose, clip = inputs

    def run():
        net.fp8_probe(x, t, ctx, None, concat_images=torch.zeros(1, device=DEV), image_clip_features=clip, ref_concat=ref, concat_smpl_render=pose)
        return net.fp8_probe_table.to(DEV)

    table = _contract(run, _dit_objs(net, inputs))[0]
    assert table.shape == (LAYERS, 6, 4) and bool((table != 0).any(dim=2).all()), "every GEMM of every layer was measured"


# ---- DiT: block, the samplers ---------------------------------------------------------------------------------------------------------------------
def _block_operands(net, inputs, T, hp, wp, Ltok):
    x, t, ctx, ref, pose, clip = inputs
    g = torch.Generator().manual_seed(3)
    hidden = torch.randn(2, Ltok, net.hidden_size, generator=g).to(DEV).to(torch.bfloat16)
    mod = (0.3 * torch.randn(2, 6 * net.hidden_size, generator=g)).to(DEV)
    cond = net._conditioning(ctx, clip)
    cos, sin = net._rope(T, hp, wp, 0, 0, x.device, 1)
    return hidden, mod, cond, cos, sin


def test_block():
    net, inputs = _net(), _inputs(SMALL)
    hidden, mod, cond, cos, sin = _block_operands(net, inputs, SMALL[0], SMALL[1] // 2, SMALL[2] // 2, 190)
    ex = net._executor()
    out = _contract(lambda: ex.block(1, hidden.clone(), mod, cond, cos, sin), _dit_objs(net, inputs, hidden=hidden, mod=mod),
                    expect_what="scail_dit_block_workspace_bytes")[0]
    assert not torch.equal(out, hidden)


@pytest.mark.parametrize("n_char", [1, 2])
def test_sample(n_char):
    """2 Euler steps: the second reuses the workspace as the first left it"""
    net, inputs = _net("toy" if n_char == 1 else "tiny2"), _inputs(SMALL, n_char=n_char)
    x, t, ctx, ref, pose, clip = inputs
    sig = torch.tensor([1.0, 0.55, 0.2])
    out = _contract(lambda: net.sample_c(x[:1], sig, 4.0, ctx, ref, pose, clip), _dit_objs(net, inputs), expect_what="scail_dit_sample_chars_workspace_bytes")[0]
    assert out.shape == x[:1].shape and not torch.equal(out, x[:1])


def test_sample_tiled(golden_dir):
    """T 6 in three 4-frame tiles, 8 x 8: den and the pair buffers"""
    import test_longclip_gpu as LC
    g, net, tiles, c, uc = LC._golden_request(golden_dir)
    x0, smp = g["x0"].to(DEV), LC._sampler(2)
    assert x0.shape[1] == 6 and len(tiles) == 3 and len(tiles[0]) == 4 and tuple(x0.shape[3:]) == (8, 8)
    out = _contract(lambda: smp.sample_hip(net, x0, c, uc, tile_indices=tiles), _dit_objs(net, (x0, c, uc)),
                    expect_what="scail_dit_sample_tiled_workspace_bytes")[0]
    assert not torch.equal(out, x0)


# ---- DiT: sequence-parallel virtual ranks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,mode,chunk_dim", [(2, "allgather", 3), (4, "ulysses", 4)])
def test_sequence_parallel_virtual_ranks(world, mode, chunk_dim):
    """every rank's workspace comes from the patched hand-out; every rank's network must still hold the weights of a fresh one"""
    import test_parallel_gpu as P
    inputs = P._inputs(2, 32, 32, 1, 64, 12, 5, seed=11)
    fresh = P._mk(TOY, LAYERS, seed=77)
    want = W.snapshot(dict(net=fresh, prepared=fresh.prepare()))
    nets = []

    def mk():
        nets.append(P._mk(TOY, LAYERS, seed=77))
        return nets[-1]

    snap = W.snapshot(dict(inputs=inputs))
    plain = P._run_ranks(world, mode, mk, inputs, chunk_dim, use_c=True)
    got = {}
    for name, fill in W.FILLS.items():
        with W.poisoned(fill) as s:
            got[name] = P._run_ranks(world, mode, mk, inputs, chunk_dim, use_c=True)
            assert len(s.workspaces) == world and all("scail_dit_sp_chars_workspace_bytes" in what for what, _ in s.workspaces)
            assert len(s.outs) == world
            s.check()
    for name, o in got.items():
        assert bool(torch.isfinite(o).all()), f"fill {name}"
        assert torch.equal(o, got["zero"]), f"fill {name} differs from fill zero in {int((o != got['zero']).sum())} values"
        assert torch.equal(o, plain), f"fill {name} differs from the plain run in {int((o != plain).sum())} values"
    W.assert_unchanged(snap)
    assert len(nets) == 4 * world
    for n in nets:
        W.assert_unchanged(want, dict(net=n, prepared=n._prepared))


# ---- DiT: stale data from another shape -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", sorted(W.FILLS), ids=str)
def test_step_after_a_larger_step_in_the_same_buffer(fill):
    net, big, small = _net(), _inputs(LARGE, seed=5), _inputs(SMALL)
    snap = W.snapshot(_dit_objs(net, (big, small))())
    with W.poisoned(W.FILLS["zero"]) as s:
        fresh = _fwd(net, small).clone()
        s.check()
    with W.poisoned(W.FILLS[fill], reuse=True) as s:
        _fwd(net, big)
        out = _fwd(net, small).clone()
        (_, first), (_, second) = s.workspaces
        assert second.data_ptr() == first.data_ptr() and second.numel() <= first.numel() and len(s.tails) == 1, "the same buffer, not refilled"
        s.check()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, fresh), f"{int((out != fresh).sum())} values differ"
    W.assert_unchanged(snap)


# ---- VAE ------------------------------------------------------------------------------------------------------------------------------------------
HL, WL = 5, 7                   # nt 35: nt % 8 = 3 (three key rows past the last frame), npad 64 (29 pad columns of S / vt)


def _vae(dim):
    import test_vae_stream_gpu as S
    return S._model(dim)


def _latent(Tl):
    import test_vae_stream_gpu as S
    return S._latent(Tl, HL, WL)


def _vae_objs(m, **inputs):
    def objs():
        c = getattr(m, "_cvae", None)
        return dict(model=m, prepared=getattr(m, "_prepared", None), keep=getattr(c, "_keep", None), **inputs)
    return objs


VAE_CASES = [("decode", 3, None), ("decode", 1, None),          # a single frame: the attention temporaries set the slot size
             ("decode", 5, 2), ("decode", 6, 2),                # chunk 2: Tl 5 = 2 + 3 (a remainder of one joins the last chunk), Tl 6 = three chunks
             ("decode_u8", 3, None), ("decode_u8", 1, None), ("decode_u8", 5, 2), ("decode_u8", 6, 2)]


@pytest.mark.parametrize("dim", [32, 96])
@pytest.mark.parametrize("entry,Tl,chunk", VAE_CASES, ids=[f"{e}-Tl{t}" + (f"-chunk{c}" if c else "") for e, t, c in VAE_CASES])
def test_vae_decode(entry, Tl, chunk, dim):
    m, z = _vae(dim), _latent(Tl)
    what = "scail_vae_decode_stream_workspace_bytes" if chunk else "scail_vae_workspace_bytes"
    out = _contract(lambda: getattr(m, entry)(z, chunk_frames=chunk), _vae_objs(m, z=z), expect_what=what)[0]
    T = 1 + 4 * (Tl - 1)
    assert out.shape == ((1, 3, T, 8 * HL, 8 * WL) if entry == "decode" else (1, T, 8 * HL, 8 * WL, 3))
    assert out.dtype == (torch.float32 if entry == "decode" else torch.uint8) and len(out.unique()) > 16


@pytest.mark.parametrize("dim", [32, 96])
def test_vae_encode(dim):
    m = _vae(dim)
    video = torch.randn(1, 3, 9, 8 * HL, 8 * WL, generator=torch.Generator().manual_seed(9)).to(DEV)
    out = _contract(lambda: m.encode(video), _vae_objs(m, video=video), expect_what="scail_vae_workspace_bytes")[0]
    assert out.shape == (1, 16, 3, HL, WL)


@pytest.mark.parametrize("dim", [32, 96])
@pytest.mark.parametrize("fill", sorted(W.FILLS), ids=str)
def test_vae_decode_after_a_longer_clip_in_the_same_buffer(fill, dim):
    m, z3, z1 = _vae(dim), _latent(3), _latent(1)
    snap = W.snapshot(_vae_objs(m, z3=z3, z1=z1)())
    with W.poisoned(W.FILLS["zero"]) as s:
        fresh = m.decode(z1).clone()
        s.check()
    with W.poisoned(W.FILLS[fill], reuse=True) as s:
        m.decode(z3)
        out = m.decode(z1).clone()
        (_, first), (_, second) = s.workspaces
        assert second.data_ptr() == first.data_ptr() and second.numel() <= first.numel() and len(s.tails) == 1, "the same buffer, not refilled"
        s.check()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, fresh), f"{int((out != fresh).sum())} values differ"
    W.assert_unchanged(snap)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
class _NoFabric:
    """a 2-rank backend that never exchanges: a refused call does not get that far, and one that did would fail here instead of waiting"""
    rank, size = 0, 2

    def all_gather_into(self, *a, **k):
        raise RuntimeError("a call that had to be refused reached the exchange")

    all_to_all = all_gather_into


def _refusal_case(entry):
    """-> (run, objs): one call of ``entry`` through the Python layers, and what it must leave alone (in / out tensors included)"""
    if entry.startswith("vae_"):
        m, z = _vae(32), _latent(3)
        video = torch.randn(1, 3, 9, 8 * HL, 8 * WL, generator=torch.Generator().manual_seed(9)).to(DEV)
        run = {"vae_encode": lambda: m.encode(video), "vae_decode": lambda: m.decode(z), "vae_decode_u8": lambda: m.decode_u8(z)}[entry]
        m.decode(_latent(1))                 # the executor and its prepared weights exist
        return run, _vae_objs(m, z=z, video=video)
    net, inputs = _net(), _inputs(SMALL)
    x, t, ctx, ref, pose, clip = inputs
    _fwd(net, inputs)                        # the executor, the conditioning and the rope tables exist
    ex = net._executor()
    if entry == "step":
        return (lambda: _fwd(net, inputs)), _dit_objs(net, inputs)
    if entry == "sample":
        x1 = x[:1].clone()
        cond, (cos, sin) = net._conditioning(ctx, clip), net._rope(SMALL[0], SMALL[1] // 2, SMALL[2] // 2, 0, 0, x.device, 1)
        return (lambda: ex.sample(x1, torch.tensor([1.0, 0.55, 0.2]), 4.0, cond, ref, pose, cos, sin)), _dit_objs(net, inputs, x1=x1)
    if entry == "block":
        hidden, mod, cond, cos, sin = _block_operands(net, inputs, SMALL[0], SMALL[1] // 2, SMALL[2] // 2, 190)
        return (lambda: ex.block(1, hidden, mod, cond, cos, sin)), _dit_objs(net, inputs, hidden=hidden, mod=mod)
    # the two sequence-parallel forms: rank 0 of 2, the upper half of the latent's rows
    from scail_amd.parallel import SequenceParallel
    T, H, Wd = SMALL[0], SMALL[1] // 2, SMALL[2]
    Ltok = _ltok(T, H, Wd)
    xch = SequenceParallel(_NoFabric(), mode="allgather").c_exchange(net.num_attention_heads, net.hidden_size, 2, Ltok, x.device)
    if entry == "step_sp":
        xs, rs, ps = x[:, :, :, :H].contiguous(), ref[:, :, :, :H].contiguous(), pose[:, :, :, :H // 2].contiguous()
        cond, (cos, sin) = net._conditioning(ctx, clip), net._rope(T, H // 2, Wd // 2, 0, 0, x.device, 1)
        return (lambda: ex.step_sp(xs, t, cond, rs, ps, cos, sin, xch)), _dit_objs(net, inputs, slabs=(xs, rs, ps))
    assert entry == "block_sp"
    hidden, mod, cond, cos, sin = _block_operands(net, inputs, T, H // 2, Wd // 2, Ltok)
    return (lambda: ex.block_sp(1, hidden, mod, cond, cos, sin, xch)), _dit_objs(net, inputs, hidden=hidden, mod=mod)


@pytest.mark.parametrize("how", W.TAMPERINGS)
@pytest.mark.parametrize("entry", ["step", "block", "sample", "step_sp", "block_sp", "vae_encode", "vae_decode", "vae_decode_u8"])
def test_refusal_enqueues_nothing(entry, how):
    """workspace_bytes one short, then the pointer moved by 128 bytes: ScailHipError, and nothing was enqueued -- the NaN-filled output is all
    NaN, the workspace holds its fill, the guards are intact, in / out tensors keep their bits.  (The tiled sampler and the two streamed
    decodes have such a test in test_longclip_gpu.py and test_vae_stream_gpu.py.)"""
    from scail_amd import lib as L
    run, objs = _refusal_case(entry)
    torch.cuda.synchronize()
    snap = W.snapshot(objs())
    with W.poisoned(W.FILLS["big"], out_fill=W.FILLS["nan"]) as s, W.tampered(s, how) as hit:
        with pytest.raises(L.ScailHipError, match="workspace"):
            run()
        torch.cuda.synchronize()
        assert len(hit) == 1, f"the call that carries the workspace was not seen: {hit}"
        assert len(s.workspaces) == 1
        assert W.holds_fill(s.workspaces[0][1], W.FILLS["big"]), f"{hit[0]} wrote to the workspace before it refused"
        for o in s.outs:
            assert W.holds_fill(o, W.FILLS["nan"]), f"{hit[0]} wrote to its output before it refused"
        s.check()
    W.assert_unchanged(snap)
    if not entry.endswith("_sp"):            # and the same call on the whole workspace does run (the sp forms would need their peers)
        with W.poisoned(W.FILLS["big"]) as s:
            run()
            s.check()
