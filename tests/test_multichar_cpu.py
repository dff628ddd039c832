"""Multi-character requests through the one-call executor, the part that needs no GPU: the character count is an argument of the
network-level C ABI (include/scail_dit.h "more than one character"), bound in scail_amd/lib.py and passed down by the Python layers;
bad character arguments are host-side returns that name the value, before any device call."""
import inspect

import pytest
import torch

CHARS_SYMBOLS = ["scail_patchify_chars", "scail_dit_chars_workspace_bytes", "scail_dit_step_chars", "scail_dit_sp_chars_workspace_bytes",
                 "scail_dit_step_sp_chars", "scail_dit_sample_chars_workspace_bytes", "scail_dit_sample_chars"]
A = 0x1000       # a fake, suitably aligned device address: validation fails before it is ever dereferenced


@pytest.fixture(scope="module")
def L():
    from scail_amd import build, lib
    build.build(verbose=False)
    lib.load()
    return lib


def test_chars_entry_points_are_bound_and_exported(L):
    lib = L.load()
    for name in CHARS_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    # every *_chars form is its base entry point + the character arguments
    extra = {"scail_patchify_chars": ("scail_patchify", 1), "scail_dit_chars_workspace_bytes": ("scail_dit_workspace_bytes", 1),
             "scail_dit_step_chars": ("scail_dit_step", 2), "scail_dit_sp_chars_workspace_bytes": ("scail_dit_sp_workspace_bytes", 1),
             "scail_dit_step_sp_chars": ("scail_dit_step_sp", 2), "scail_dit_sample_chars_workspace_bytes": ("scail_dit_sample_workspace_bytes", 1),
             "scail_dit_sample_chars": ("scail_dit_sample", 2)}
    for name, (base, n) in extra.items():
        assert len(L.SIGNATURES[name]) == len(L.SIGNATURES[base]) + n, name
    assert L.ABI_VERSION >= 7 and lib.scail_abi_version() == L.ABI_VERSION
    for name in ("scail_dit_chars_workspace_bytes", "scail_dit_sp_chars_workspace_bytes", "scail_dit_sample_chars_workspace_bytes"):
        assert getattr(lib, name).restype is L._i64, name


def test_python_layers_take_the_character_count():
    from scail_amd import ops
    from scail_amd.cstep import CStep
    from scail_amd.dit import DiffusionTransformer
    for fn in (CStep.step, CStep.step_sp, CStep.sample, CStep.workspace_bytes, ops.patchify):
        p = inspect.signature(fn).parameters
        assert "n_char" in p and p["n_char"].default == 1, fn
    assert "n_char" in inspect.signature(DiffusionTransformer._rope).parameters


def test_patchify_chars_argument_checks_are_host_side(L):
    ok = dict(n_batch=2, n_ref=1, n_pose=1, n_char=2, T=3, H=8, W=12, kpad=128)

    def call(x=A, ref=A, pose=A, tok=A, **kw):
        a = dict(ok, **kw)
        L.call("scail_patchify_chars", x, ref, pose, tok, a["n_batch"], a["n_ref"], a["n_pose"], a["n_char"], a["T"], a["H"], a["W"], a["kpad"], None)

    for bad in (0, -1, 65):
        with pytest.raises(L.ScailHipError, match=rf"n_char must be 1\.\.64, got {bad}\b"):
            call(n_char=bad)
    with pytest.raises(L.ScailHipError, match="multiples of 4"):
        call(H=6)
    with pytest.raises(L.ScailHipError, match="kpad must be"):
        call(kpad=72)
    with pytest.raises(L.ScailHipError, match="cond batch must be 1 or n_batch"):
        call(n_batch=4, n_ref=2)
    for kw in (dict(x=A + 4), dict(ref=A + 2), dict(pose=A + 2), dict(tok=A + 8)):
        with pytest.raises(L.ScailHipError, match="pointer alignment"):
            call(**kw)
    call(n_batch=0)          # an empty problem is accepted and launches nothing


def test_executor_character_checks_name_the_value(L):
    """n_char and the pose frame count are checked first, so the checks run without a handle (and without a device)."""
    lib = L.load()

    def step(n_char, pose_frames, T=4):
        L.call("scail_dit_step_chars", None, A, A, A, A, 1, A, 1, n_char, pose_frames, A, A, A, 2, T, 8, 8, 0, A, 1 << 30, None)

    def sample(n_char, pose_frames, T=4):
        L.call("scail_dit_sample_chars", None, A, A, A, 2, 4.0, A, A, A, n_char, pose_frames, A, A, T, 8, 8, A, 1 << 30, None)

    for fn, who in ((step, "scail_dit_step"), (sample, "scail_dit_sample")):
        with pytest.raises(L.ScailHipError, match=who + r": n_char must be 1\.\.64, got 0\b"):
            fn(0, 0)
        with pytest.raises(L.ScailHipError, match=who + r": n_char must be 1\.\.64, got 65\b"):
            fn(65, 65 * 4)
        with pytest.raises(L.ScailHipError, match=r"n_char \* T = 2 \* 4 frames, got 4\b"):
            fn(2, 4)
        with pytest.raises(L.ScailHipError, match="null"):       # good character arguments: the next check (no handle) answers
            fn(2, 8)
    # the workspace queries refuse the same values (-1), and a null handle
    assert lib.scail_dit_chars_workspace_bytes(None, 2, 4, 8, 8, 2) == -1
    assert lib.scail_dit_sp_chars_workspace_bytes(None, 0, 2, 2, 4, 8, 8, 2) == -1
    assert lib.scail_dit_sample_chars_workspace_bytes(None, 4, 8, 8, 2) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_multi_character_request_has_no_cpu_fallback():
    from scail_amd import lib as L
    from scail_amd.dit import DiffusionTransformer
    net = DiffusionTransformer(transformer_args=dict(model_parallel_size=1), hidden_size=128, num_layers=1, num_attention_heads=1, text_dim=64,
                               time_embed_dim=128, time_freq_dim=256, inner_hidden_size=256, share_adaln=True, use_i2v_clip=True, device="cpu")
    with pytest.raises(L.ScailHipError, match="GPU"):
        net(torch.zeros(2, 1, 16, 4, 4), timesteps=torch.zeros(2), context=torch.zeros(2, 4, 64), concat_images=torch.zeros(1),
            ref_concat=torch.zeros(1, 2, 16, 4, 4), concat_smpl_render=torch.zeros(1, 2, 16, 2, 2), image_clip_features=torch.zeros(1, 3, 1280))
