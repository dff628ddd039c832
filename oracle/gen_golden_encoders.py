"""tests/golden/encoders_tiny.npz from the REAL reference T5Encoder / VisionTransformer (CPU fp32).
Build-container only.  Usage: python oracle/gen_golden_encoders.py [planted]   (``planted``: encoders_planted.npz alone)"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shims  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
T5 = dict(vocab=100, dim=128, dim_attn=128, dim_ffn=256, num_heads=2, num_layers=2, num_buckets=32)
VIT = dict(image_size=56, patch_size=14, dim=192, mlp_ratio=4, out_dim=64, num_heads=2, num_layers=3)


def bfr(sd):
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


def gen_planted(clip, umt5):
    """tests/golden/encoders_planted.npz: the real reference classes on the PLANTED towers and inputs of tests/enc_wiring.py (that
    module's seeded draws, nothing of the reference's).  The file holds the seed, the inputs and the outputs; the weights are drawn
    again from the seed.  "pre" is what CLIPModel.visual hands its tower for the planted clip: the method itself, run on a stand-in
    for ``self`` that carries image_size 70, returns the tower's input, and normalises as torchvision's Normalize does with the
    constants of clip.py:447-448 (torchvision is a stub in this container)."""
    import types
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import enc_wiring as W
    enc = umt5.T5Encoder(shared_pos=False, dropout=0.0, **W.T5CFG).eval()
    enc.load_state_dict(W.planted_t5(), strict=True)
    inp = W.planted_t5_inputs()
    vcfg = {k: v for k, v in W.VITCFG.items()}
    vit = clip.VisionTransformer(pool_type="token", pre_norm=True, post_norm=False, activation="gelu", **vcfg).eval()
    vit.load_state_dict(W.planted_vit(), strict=True)
    imgs = W.planted_images()
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)
    me = types.SimpleNamespace(dtype=torch.float32, model=types.SimpleNamespace(image_size=W.VITCFG["image_size"], visual=lambda v, use_31_block: v),
                               transforms=types.SimpleNamespace(transforms=[lambda t: t.sub_(mean).div_(std)]))
    video = W.planted_clip()
    with torch.no_grad():
        t5_out = enc(inp["ids"], inp["mask"])
        vit_out = vit(imgs, use_31_block=True)
        pre = clip.CLIPModel.visual(me, [video.clone()])
    b16 = lambda t: t.to(torch.bfloat16).view(torch.int16).numpy()       # the inputs are bf16-exact: stored as bit patterns
    np.savez_compressed(os.path.join(OUT, "encoders_planted.npz"), seed=W.SEED, ids=inp["ids"].numpy(), mask=inp["mask"].numpy(),
                        imgs=b16(imgs), clip=b16(video), t5_out=t5_out.numpy(), vit_out=vit_out.numpy(), pre=pre.numpy())
    print("planted: t5", tuple(t5_out.shape), float(t5_out.abs().mean()), "vit", tuple(vit_out.shape), float(vit_out.abs().mean()),
          "pre", tuple(pre.shape), float(pre.abs().mean()))


def main():
    torch.cuda.current_device = lambda: "cpu"           # default-arg evaluated at import (umt5.py:480, clip.py:492)
    if "ftfy" not in sys.modules:
        sys.modules["ftfy"] = MagicMock()
    ref_shims.load_reference()
    from sgm.modules.encoders import clip, umt5
    gen_planted(clip, umt5)
    if sys.argv[1:] == ["planted"]:
        return
    torch.manual_seed(11)
    enc = umt5.T5Encoder(shared_pos=False, dropout=0.0, **T5).eval()
    enc.load_state_dict(bfr(enc.state_dict()))
    ids = torch.randint(0, 100, (2, 40))
    mask = torch.ones(2, 40, dtype=torch.long)
    mask[1, 17:] = 0
    with torch.no_grad():
        t5_out = enc(ids, mask)
    vit = clip.VisionTransformer(pool_type="token", pre_norm=True, post_norm=False, activation="gelu", **VIT).eval()
    vit.load_state_dict(bfr(vit.state_dict()))
    imgs = torch.randn(2, 3, 56, 56).to(torch.bfloat16).float()
    with torch.no_grad():
        vit_out = vit(imgs, use_31_block=True)
    np.savez_compressed(os.path.join(OUT, "encoders_tiny.npz"), ids=ids.numpy(), mask=mask.numpy(), t5_out=t5_out.numpy(),
                        imgs=imgs.numpy(), vit_out=vit_out.numpy(),
                        # weights are bf16-exact: store the bf16 bit patterns (uint16) to halve the fixture
                        **{"t5." + k: v.to(torch.bfloat16).view(torch.int16).numpy() for k, v in enc.state_dict().items()},
                        **{"vit." + k: v.to(torch.bfloat16).view(torch.int16).numpy() for k, v in vit.state_dict().items()})
    print("t5", tuple(t5_out.shape), float(t5_out.abs().mean()), "vit", tuple(vit_out.shape), float(vit_out.abs().mean()))


if __name__ == "__main__":
    main()
