"""The workspace contract of the two C executors (csrc/dit_step.hip, csrc/vae_exec.hip), as a test helper.

Both executors carve a caller-owned workspace into regions and reuse them across launches, layers, chunks and calls.  What they promise the
caller: a call reads no workspace byte before writing it, needs no more than its ``*_workspace_bytes`` query answers, writes nothing outside
the workspace and its outputs, and leaves every input as it was.  This module makes each of those observable:

  * ``guarded(need, fill, device)``: exactly ``need`` bytes, 256-byte aligned, filled with ``fill``, between two 64 KiB bands of 0xA5 inside one
    allocation; the checker it returns asserts that the bands are intact.
  * ``FILLS``: the three byte patterns a workspace is run under.  A result that depends on a never-written byte differs between them: 0xFF is
    NaN in every element type the workspaces hold, 0x47 a large finite number (NaN can be masked by an fmaxf; the finite fill is not), 0x00 what
    a fresh allocation tends to look like.
  * ``poisoned(fill)``: hands every workspace of CStep / CVae out through ``guarded`` at exactly the queried size (CStep._ws_for, CVae._workspace,
    CVae._stream_workspace), and every buffer the two bindings allocate with ``torch.empty`` -- the ``out`` of a step, the fp32 / uint8 video,
    the fp8 probe's scratch -- through ``guarded_like``.  Nothing in scail_amd is edited: the three methods and the bindings' ``torch`` name are
    monkeypatched for the duration of the ``with`` block.
  * ``tampered(session, how)``: rewrites the (workspace pointer, workspace bytes) pair of every library call on its way through ``lib.call`` --
    one byte short, or moved by 128 bytes -- so that a refusal is reached through the project's own Python layers.
  * ``snapshot`` / ``assert_unchanged``: bitwise CPU copies of every tensor reachable from the given objects (modules, dicts, lists, tuples).

What the regions hold (read off the layout code before the first poisoned run): ``Ws``, ``BlockWs`` and ``SampleWs`` of dit_step.hip are bf16
activations (tok, h, xn, qkv, att, ff, vt, xf, tokout), fp32 tables (temb, e1, emb, adaln, mod, emb2, fin, xin, v, den), e4m3 codes (xq) and
fp32 or E8M0 scales (sx); dit_block_sp uses xn, qkv, att and vt of the same BlockWs and nothing else of the workspace (its exchange buffers are
the caller's).  The ``Arena`` slots and the ``StreamPlan`` carry areas of vae_exec.hip are bf16 activations.  No region holds an index, an offset
or a pointer that a kernel dereferences, so every region takes all three fills: a poisoned value can make a result wrong or NaN, never an
address."""
import contextlib
import math
import threading

import torch

GUARD = 64 * 1024
BAND = 0xA5
ALIGN = 256
FILLS = {"zero": 0x00, "nan": 0xFF, "big": 0x47}
ELEMENT_TYPES = ("fp32", "bf16", "e4m3", "e8m0")


def decode_fill(byte: int, kind: str) -> float:
    """the value of an element whose every byte is ``byte``, in one of the four element types the workspaces hold"""
    if kind == "fp32":
        return float(torch.tensor([byte] * 4, dtype=torch.uint8).view(torch.float32)[0])
    if kind == "bf16":
        return float(torch.tensor([byte] * 2, dtype=torch.uint8).view(torch.bfloat16)[0])
    if kind == "e4m3":                     # OCP e4m3fn: 1-4-3, bias 7, no infinities, S.1111.111 = NaN
        s, e, m = byte >> 7, (byte >> 3) & 15, byte & 7
        if e == 15 and m == 7:
            return math.nan
        v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        return -v if s else v
    if kind == "e8m0":                     # OCP MX scale: 2^(byte - 127), 0xFF = NaN
        return math.nan if byte == 0xFF else 2.0 ** (byte - 127)
    raise ValueError(kind)


def _sync(t):
    if t.device.type == "cuda":
        torch.cuda.synchronize(t.device)


def _first_damage(band):
    bad = (band != BAND).nonzero()
    return None if bad.numel() == 0 else int(bad[0])


def guarded(need: int, fill: int, device):
    """(uint8 view of exactly ``need`` bytes filled with ``fill``, check): the view's data_ptr() is 256-byte aligned and it lies between two
    bands of at least 64 KiB of 0xA5 in one allocation.  ``check(what)`` synchronises and asserts both bands intact; it names the first
    damaged byte relative to the end of the view (behind it) or to its start (in front of it)."""
    raw = torch.empty(need + 2 * GUARD + ALIGN, device=device, dtype=torch.uint8)
    off = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN          # from the pointer: a CPU allocation is only 64-byte aligned
    raw.fill_(BAND)
    view = raw[off:off + need]
    view.fill_(fill)
    assert view.data_ptr() % ALIGN == 0 and view.numel() == need

    def check(what="workspace"):
        _sync(raw)
        hi = _first_damage(raw[off + need:])
        assert hi is None, f"{what}: write past the end: first damaged byte at end + {hi} (of {need} bytes)"
        lo = _first_damage(raw[:off].flip(0))
        assert lo is None, f"{what}: write in front of the start: first damaged byte at start - {lo + 1}, end - {need + lo + 1}"

    return view, check


def guarded_like(t: torch.Tensor, fill: int):
    """(a tensor of t's shape and dtype in guarded memory, every byte ``fill``; its check)"""
    view, check = guarded(t.numel() * t.element_size(), fill, t.device)
    return view.view(t.dtype).view(t.shape), check


def holds_fill(t: torch.Tensor, fill: int) -> bool:
    _sync(t)
    return bool((t.contiguous().view(-1).view(torch.uint8) == fill).all())


class Session:
    """what ``poisoned`` handed out: ``workspaces`` [(what, view)], ``outs`` (the guarded torch.empty results), and their checks"""

    def __init__(self, fill, out_fill, reuse):
        self.fill, self.out_fill, self.reuse = fill, fill if out_fill is None else out_fill, reuse
        self.workspaces, self.outs, self._checks, self.tails = [], [], [], []
        self._kept = None
        self._lock = threading.Lock()          # the virtual ranks of a sequence-parallel run are threads

    def workspace(self, need, device, what):
        if self.reuse and self._kept is not None and self._kept.numel() >= need and self._kept.device == torch.device(device):
            # stale data from an earlier call: the same memory, not refilled, exactly ``need`` bytes of it; what lies behind is kept as it is
            ws, tail = self._kept[:need], self._kept[need:]
            _sync(ws)
            with self._lock:
                self.tails.append((what, tail, tail.to("cpu", copy=True)))
        else:
            ws, check = guarded(need, self.fill, device)
            with self._lock:
                self._checks.append((what, check))
            if self.reuse:
                self._kept = ws
        with self._lock:
            self.workspaces.append((what, ws))
        return ws

    def like(self, t, what="output"):
        g, check = guarded_like(t, self.out_fill)
        with self._lock:
            self.outs.append(g)
            self._checks.append((what, check))
        return g

    def check(self):
        """after a synchronise: every guard band intact, and (reuse) nothing written behind the ``need`` bytes of a reused workspace"""
        assert self.workspaces, "no workspace was handed out: the executor did not run through the patched hand-out points"
        for what, check in self._checks:
            check(what)
        for what, tail, before in self.tails:
            _sync(tail)
            bad = (tail.cpu() != before).nonzero()
            assert bad.numel() == 0, f"{what}: write past the end of a reused workspace: first damaged byte at end + {int(bad[0])}"


class _TorchProxy:
    """stands in for the name ``torch`` of a binding module: ``empty`` hands out guarded memory, everything else is torch's"""

    def __init__(self, session):
        self._session = session

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        return self._session.like(torch.empty(*shape, **kw))


@contextlib.contextmanager
def poisoned(fill: int, out_fill=None, reuse=False):
    """CStep / CVae take every workspace from ``guarded(need, fill)`` at exactly the queried size and every buffer of their own from
    ``guarded_like(.., out_fill or fill)``.  ``reuse``: a later request that fits the first workspace gets its first ``need`` bytes, as they
    are.  Yields the Session; call its ``check()`` before leaving."""
    import pytest
    from scail_amd import cstep, cvae
    from scail_amd import lib as L
    s = Session(fill, out_fill, reuse)

    def ws_for(self, need, device, what):
        if need < 0:
            raise L.ScailHipError(f"{what}: the executor has no workspace for this request (bad shape / mode)")
        self._ws = s.workspace(need, device, what)
        return self._ws

    def vae_ws(self, T, H, W):
        need = L.load().scail_vae_workspace_bytes(self._h, T, H, W)
        if need < 0:
            raise ValueError("video needs T = 1 + 4n frames and H, W multiples of 8")
        self._ws = s.workspace(need, self._dev, f"scail_vae_workspace_bytes (T {T}, H {H}, W {W})")
        return self._ws

    def vae_stream_ws(self, chunk, h, w):
        need = L.load().scail_vae_decode_stream_workspace_bytes(self._h, chunk, h, w)
        if need < 0:
            raise ValueError(f"chunk_frames must be at least 2 latent frames, got {chunk}")
        self._ws = s.workspace(need, self._dev, f"scail_vae_decode_stream_workspace_bytes (chunk {chunk}, h {h}, w {w})")
        return self._ws

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(cstep.CStep, "_ws_for", ws_for)
        mp.setattr(cvae.CVae, "_workspace", vae_ws)
        mp.setattr(cvae.CVae, "_stream_workspace", vae_stream_ws)
        proxy = _TorchProxy(s)
        mp.setattr(cstep, "torch", proxy)
        mp.setattr(cvae, "torch", proxy)
        yield s


TAMPERINGS = ("short", "shifted")


@contextlib.contextmanager
def tampered(session: Session, how: str):
    """Every library call that passes the session's latest workspace as (pointer, bytes) gets, instead, (pointer, bytes - 1) ("short") or
    (pointer + 128, bytes) ("shifted": no longer 256-byte aligned; were the refusal missing, the over-run of 128 bytes would land in the
    band).  Yields the list of the calls that were rewritten."""
    import pytest
    from scail_amd import lib as L
    assert how in TAMPERINGS
    orig, hit = L.call, []

    def call(name, *args):
        if not session.workspaces:
            return orig(name, *args)
        _, ws = session.workspaces[-1]
        ptr, n = ws.data_ptr(), ws.numel()
        args = list(args)
        for i in range(len(args) - 1):
            if isinstance(args[i], int) and isinstance(args[i + 1], int) and (args[i], args[i + 1]) == (ptr, n):
                args[i], args[i + 1] = (ptr, n - 1) if how == "short" else (ptr + 128, n)
                hit.append(name)
                break
        return orig(name, *args)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "call", call)
        yield hit


def _tensors(obj, path, out, seen):
    if isinstance(obj, torch.Tensor):
        if id(obj) not in seen:
            seen.add(id(obj))
            out.append((path, obj))
    elif isinstance(obj, torch.nn.Module):
        for n, p in list(obj.named_parameters()) + list(obj.named_buffers()):
            _tensors(p.detach(), f"{path}.{n}", out, seen)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _tensors(v, f"{path}[{k!r}]", out, seen)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _tensors(v, f"{path}[{i}]", out, seen)


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).to("cpu", copy=True)


def snapshot(objs: dict):
    """CPU copies of the bytes of every tensor reachable from ``objs`` (name -> tensor / module / dict / list / tuple; anything else is
    skipped).  -> [(path, tensor, bytes)]"""
    found = []
    _tensors(objs, "", found, set())
    assert found, "nothing to snapshot"
    for _, t in found[:1]:
        _sync(t)
    return [(path, t, _bits(t)) for path, t in found]


def assert_unchanged(snap, objs=None):
    """every snapshotted tensor holds the bytes it held (``objs``: compare these objects, path by path, with the snapshot instead)"""
    if objs is None:
        now = [(path, t) for path, t, _ in snap]
    else:
        now = []
        _tensors(objs, "", now, set())
        assert [p for p, _ in now] == [p for p, _, _ in snap], "the two object trees differ"
    for (path, _, before), (_, t) in zip(snap, now):
        _sync(t)
        assert torch.equal(_bits(t), before), f"{path} was changed by the call"
