"""The convolution dispatch of csrc/conv.hip (conv_choose, one statement behind the launches and the host-only queries) against the table
recorded at the commit before it existed (tests/golden/conv_dispatch_parent.json, written by tools/conv_dispatch_table.py): for 10 680
geometries on both sides of every threshold, scail_conv3d_kernel_for answers what it answered, and the kernel that
scail_conv3d_kernel_name_for names belongs to the family the old test helper (tests/vae_stream_dispatch._conv as it was) put the launch in.

The 1 318 entries of the table's "corrected" list are cases where that helper was wrong about the parent's conv3d_impl; the table carries the
right class (each kind checked by hand against the parent's code) and the helper's:
  * ldc = N + 4 (468; the helper had no ldc argument and answered for ldc = N): the generated kernels and the direct-gather kernel need
    ldc % 8 == 0, so those shapes run the halo kernel, the halo kernel behind the upsample or the implicit GEMM;
  * ldc = N + 4 or N + 8, next-norm form (another 40): one launch needs dense outputs, ldc == N == 96; the call is the plain kernel + the pass;
  * scail_conv3d_cl_norm of a 3x3x3 convolution behind `ups` (128): the helper said "halo norm"; the halo kernel does not take `ups`, the
    call is rejected, and a ResidualBlock would run the plain convolution + the pass;
  * stride (1, 2, 2) (770 over the three forms): outside the helper's reach, it had no stride argument -- conv_s2_kernel where Cin % 32 == 0,
    N % 96 == 0 and there is no residual, else the implicit GEMM.
The direct-gather rule's `lds <= 150 KB` term cannot decide for any shape: the instantiated shapes need at most 96 KB.  Needs no GPU."""
import ctypes as C
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch_parent.json")


def library():
    from scail_amd import build
    build.build(verbose=False)
    from scail_amd import lib as L
    return L.load()


def kernel_name(lib, geom, ldc, ldr, form):
    from scail_amd import lib as L
    buf = C.create_string_buffer(128)
    L.call("scail_conv3d_kernel_name_for", geom, ldc, ldr, form, buf, len(buf))
    return buf.value.decode()


def family(name, form):
    """the old helper's class of a kernel name"""
    conv, _, norm_pass = name.partition(" + ")
    assert norm_pass in ("", "scail_rms_silu") and (not norm_pass or form == 2), name
    dual = form == 2 and not norm_pass
    if conv.startswith("scail_conv4"):
        return "generated dual:4" if dual else "generated norm" if form == 1 else "generated"
    args = [a.strip() for a in re.fullmatch(r"conv_\w+_kernel<(.*?)>( x 2)?", conv).group(1).split(",")]
    if conv.startswith("conv_halo_kernel"):          # <EPI, CS, NWB, SWZ, BN = 96, NF = 1, KT = 3, UPS = false, PF = 0>
        nf = args[5] if len(args) > 5 else "1"
        return "halo ups" if args[7:8] == ["true"] else f"halo norm:{nf}" if args[0] == "4" else f"halo:{nf}"
    if conv.startswith("conv_direct_kernel"):
        assert (args[2:3] == ["true"]) == dual
        return "generated dual:2" if dual else "direct"
    assert not dual
    return {"conv_igemm_kernel": "igemm", "conv_s2_kernel": "s2"}[conv.split("<")[0]]


def classes_of(lib, row):
    """[plain, conv + norm as a ResidualBlock runs it, next-norm] classes of a table row (None: the form does not exist)"""
    import conv_dispatch_table as T
    N, resid, ldc = row[1], row[9], row[10]
    geom = C.cast((C.c_int32 * 21)(*T.geom_of(row)), C.c_void_p)
    ldr = N if resid else 0
    plain = family(kernel_name(lib, geom, ldc, ldr, 0), 0)
    norm = None
    if not resid:
        norm = family(kernel_name(lib, geom, ldc, 0, 1), 1) if lib.scail_conv3d_norm_fused_for(geom, ldc) else plain
    return [plain, norm, family(kernel_name(lib, geom, ldc, ldr, 2), 2)]


def test_every_row_answers_as_the_parent_did():
    import conv_dispatch_table as T
    lib = library()
    classes, corrected, answers = T.read(TABLE)
    grid = T.grid()
    assert len(answers) == len(grid) == 10680 and len(corrected) == 1318
    bad = []
    for i, (r, a) in enumerate(zip(grid, answers)):
        geom = C.cast((C.c_int32 * 21)(*T.geom_of(r)), C.c_void_p)
        ks = [lib.scail_conv3d_kernel_for(geom, r[10], r[1] if r[9] else 0, m) for m in (0, 1, 2)]
        want = [classes[c] for c in a[3:]]
        got = classes_of(lib, r)
        if ks != a[:3] or got != want:
            bad.append((i, r, ks, a[:3], got, want))
    assert not bad, f"{len(bad)} rows differ, the first: {bad[:5]}"


def test_the_issue_examples():
    """the geometries the change was specified with, by name"""
    import conv_dispatch_table as T
    lib = library()

    def name(Cin, N, k, To, H, W, form=0, resid=0, ups=0, ot_mul=1):
        kt = T.KERNELS[k][0]
        row = [Cin, N, k, To, To, H, W, kt - 1, ups, resid, N, 0, ot_mul, 0]
        return kernel_name(lib, C.cast((C.c_int32 * 21)(*T.geom_of(row)), C.c_void_p), N, N if resid else 0, form)

    assert name(96, 96, 0, 5, 16, 16) == "scail_conv4c_e0"
    assert name(96, 96, 0, 1, 16, 16) == "conv_halo_kernel<0, 32, 1, false, 96>"
    assert name(32, 64, 0, 5, 16, 16, form=1) == "conv_halo_kernel<4, 32, 1, false, 96, 2>"
    assert name(192, 192, 0, 5, 16, 16, form=1) == "rejected" and name(192, 192, 0, 5, 16, 16) == "scail_conv4_e0"
    assert name(96, 96, 0, 5, 16, 16, form=2, resid=1) == "scail_conv4c_e5" and name(96, 96, 0, 5, 16, 16, form=3, resid=1) == "scail_conv4c_e6"
    assert name(192, 96, 1, 5, 16, 16, ups=1) == "scail_conv4u_e0"
    assert name(64, 32, 1, 1, 16, 16, ups=1) == "conv_igemm_kernel<0, 64, 4, 1>"
    assert name(64, 128, 3, 81, 12, 16) == "conv_direct_kernel<6, 4>"
    assert name(64, 128, 3, 8, 12, 16) == "conv_igemm_kernel<0, 128, 2, 2>"
    assert name(96, 8, 0, 5, 16, 16) == "scail_conv4cn_e0"
    assert name(8, 96, 0, 17, 16, 16) == "conv_direct_kernel<14, 3>"
    assert name(8, 96, 0, 17, 16, 16, form=2) == "conv_direct_kernel<14, 3, true>"
    assert name(96, 96, 2, 5, 16, 16, ot_mul=2) == "conv_igemm_kernel<0, 96, 4, 1>"
    assert name(64, 384, 3, 81, 12, 16) == "conv_direct_kernel<6, 6> x 2"
    assert name(96, 96, 0, 1, 16, 16, form=2, resid=1) == "conv_halo_kernel<3, 32, 1, false, 96> + scail_rms_silu"
    stride2 = [96, 96, 1, 4, 4, 40, 56, 0, 0, 0, 96, 1, 1, 0]
    assert kernel_name(lib, C.cast((C.c_int32 * 21)(*T.geom_of(stride2)), C.c_void_p), 96, 0, 0) == "conv_s2_kernel<1>"


def test_the_decoder_walk_is_unchanged():
    """tests/vae_stream_dispatch.py now asks the library for every name; for the cases tests/test_vae_stream_gpu.py streams, chunk and
    clip still pick the same kernels, as the restated rules said before"""
    import vae_stream_dispatch as D
    from scail_amd.wan_vae import WanVAE_
    library()
    for dim in (32, 96):
        m = WanVAE_(dim=dim, z_dim=16, device="cpu")
        for Tl, hl, wl, chunk in [(7, 6, 8, c) for c in (2, 3, 4, 5, 6)] + [(2, 6, 8, 2), (7, 5, 9, 2), (7, 5, 9, 3)]:
            assert D.dispatch_differences(m, Tl, hl, wl, chunk) == []
