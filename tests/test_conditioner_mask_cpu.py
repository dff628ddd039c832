"""The precondition of scail_attn_small (include/scail_hip.h): every key mask it is handed has at least one unmasked key per batch element; a
fully masked row has max = -inf and comes back as NaN.  The only masks the kernel sees are the tokenizer's attention masks: the conditioner hands
the prompt strings to T5EncoderModel.forward, which goes through encode_text -- the tokenizer with add_special_tokens=True, so `</s>` is always
there, the empty (unconditional) prompt included -- and from there unchanged through T5Encoder.forward to every layer's attention; the CLIP tower
passes no mask.  Pinned here on a tiny SentencePiece model trained inside the test, with the encoder itself replaced by a recorder (the real one
runs on the GPU: tests/test_encoders_gpu.py)."""
import io
import sys
import types

import pytest
import torch
from torch import nn

from scail_amd import conditioner as C
from scail_amd import tokenizer as T
from scail_amd import umt5


@pytest.fixture(scope="module")
def sp_model(tmp_path_factory):
    spm = pytest.importorskip("sentencepiece")
    corpus = ["the girl is dancing in the street", "a man walks his dog", "two people are dancing together",
              "the dog runs in the park", "a woman is singing a song"] * 20
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=model, vocab_size=40, model_type="unigram", hard_vocab_limit=False, minloglevel=2,
                                   pad_id=0, eos_id=1, unk_id=2, bos_id=-1)
    p = tmp_path_factory.mktemp("sp") / "spiece.model"
    p.write_bytes(model.getvalue())
    return str(p)


class _Recorder(nn.Module):
    """stands where T5Encoder stands: records the mask that would reach scail_attn_small in every layer"""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.masks = []

    def forward(self, ids, mask=None):
        self.masks.append(mask.clone())
        return torch.ones(ids.shape[0], ids.shape[1], 4)


def _text_model(sp_model, seq_len, **kw):
    m = umt5.T5EncoderModel.__new__(umt5.T5EncoderModel)          # (the constructor would allocate the XXL encoder)
    nn.Module.__init__(m)
    m.max_length, m.varlen_text, m.uncond_text_length, m.cond_length_multiple = seq_len, kw.get("varlen_text", False), kw.get("uncond_text_length", 1), 1
    m.model = _Recorder()
    m.tokenizer = T.HuggingfaceTokenizer(name=sp_model, seq_len=seq_len, clean="whitespace")
    return m


@pytest.fixture()
def cpu_row_affine(monkeypatch):
    monkeypatch.setattr(umt5.ops, "row_affine", lambda ctx, rowscale=None: ctx * rowscale.view(ctx.shape[0], ctx.shape[1], 1))


@pytest.mark.parametrize("seq_len", [1, 2, 16])
def test_every_mask_the_text_encoder_sees_has_a_valid_key(sp_model, cpu_row_affine, seq_len):
    m = _text_model(sp_model, seq_len)
    prompts = ["", " ", "\n\t ", "a man walks his dog", "the dog runs in the park " * 10]
    z = m(prompts)                                                  # the conditioner's call: strings
    (mask,) = m.model.masks
    assert mask.shape == (len(prompts), seq_len) and bool((mask.sum(-1) >= 1).all())
    assert mask.sum(-1).tolist()[:3] == [1, 1, 1] and int(mask[4].sum()) == seq_len          # empty prompts are `</s>` alone; truncation keeps it
    assert bool((mask[:, 0] == 1).all()) and bool((mask[:, 1:] <= mask[:, :-1]).all())      # a prefix mask
    assert z.shape == (len(prompts), seq_len, 4) and torch.equal(z[..., 0], mask.float())


def test_the_conditioner_and_the_unconditional_prompt(sp_model, cpu_row_affine):
    m = _text_model(sp_model, 12)
    stub = types.ModuleType("_stub_text_embedder")
    stub.make = lambda: m
    sys.modules["_stub_text_embedder"] = stub
    try:
        cond = C.GeneralConditioner([{"target": "_stub_text_embedder.make", "input_key": "txt"}])
        batch, batch_uc = C.get_batch(["txt"], {"prompt": "a woman is singing", "negative_prompt": ""}, [2], device="cpu")
        c, uc = cond.get_unconditional_conditioning(batch, batch_uc)
    finally:
        del sys.modules["_stub_text_embedder"]
    cm, um = m.model.masks
    assert cm.shape == um.shape == (2, 12) and bool((cm.sum(-1) >= 2).all()) and um.sum(-1).tolist() == [1, 1]
    assert c["crossattn"].shape == uc["crossattn"].shape == (2, 12, 4)
    # varlen_text: the empty prompt is cut to uncond_text_length rows, of which the first is its one valid key
    v = _text_model(sp_model, 12, varlen_text=True, uncond_text_length=1)
    assert v([""]).shape == (1, 1, 4) and v.model.masks[0].sum(-1).tolist() == [1]


def test_without_special_tokens_the_empty_prompt_would_be_fully_masked(sp_model):
    """what the precondition guards against: the same tokenizer without `</s>` gives the empty prompt no valid key at all"""
    tok = T.HuggingfaceTokenizer(name=sp_model, seq_len=8, clean="whitespace")
    assert tok([""], return_mask=True, add_special_tokens=False)[1].sum(-1).tolist() == [0]
    assert tok([""], return_mask=True, add_special_tokens=True)[1].sum(-1).tolist() == [1]
