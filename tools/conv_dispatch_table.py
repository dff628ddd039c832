"""Record the convolution dispatch of a checkout as a table: tests/golden/conv_dispatch_parent.json (names and integers only).

Run ONCE, in a checkout of the commit BEFORE csrc/conv.hip got its one choice function (33ad47a), where the kernel choice was still stated by
scail_conv3d_kernel_for, by conv3d_impl and by tests/vae_stream_dispatch._conv separately:

    python tools/conv_dispatch_table.py tests/golden/conv_dispatch_parent.json

For every geometry of the grid below it records that commit's scail_conv3d_kernel_for answers (modes 0, 1, 2) and, where the old test helper
can express the geometry (stride 1, 'same' padding), its classification for the three call forms.  tests/test_conv_dispatch_cpu.py holds
the library of every later commit against the table.  Rows where the old helper was wrong about conv3d_impl carry the corrected class and
keep the helper's answer in "corrected": [row, form, the class it gave] (--correct, run at the commit that added the name query, wrote them;
each kind was checked by hand against the parent's conv3d_impl and is listed in the test's docstring).  Needs no GPU."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = [(3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1)]
CINS = [8, 16, 32, 48, 64, 96, 192]
NS = [8, 16, 24, 32, 40, 48, 64, 96, 128, 192, 384]
TOS = [1, 2, 3, 5]
COLUMNS = ["Cin", "N", "kernel", "Ti", "To", "H", "W", "pt", "ups", "resid", "ldc", "stride2", "ot_mul", "ot_off"]


def grid():
    """rows of COLUMNS; H, W: the INPUT extent (the output's is twice that behind `ups`, half of it with stride2); kernel: index into KERNELS"""
    rows = []

    def add(Cin, N, ki, To, H, W, ups=0, resid=0, dldc=0, stride2=0, ot_mul=1, ot_off=0, carried=False):
        kt = KERNELS[ki][0]
        Ti, pt = (To + kt - 1, 0) if carried else (To, kt - 1)        # a streamed chunk's carried frames / causal padding
        rows.append([Cin, N, ki, Ti, To, H, W, pt, ups, resid, N + dldc, stride2, ot_mul, ot_off])

    for ki in range(4):
        for Cin in CINS:
            for N in NS:
                for resid in (0, 1):
                    for To in TOS:                                   # one frame / one pair / an odd pair / several
                        for ups in (0, 1):
                            add(Cin, N, ki, To, 16, 16, ups, resid)
                    for To in (1, 5):                                # row strides that are no multiple of 8, and padded ones
                        for dldc in (4, 8):
                            add(Cin, N, ki, To, 16, 16, 0, resid, dldc)
                            if ki == 1:
                                add(Cin, N, ki, To, 16, 16, 1, resid, dldc)
                if KERNELS[ki][0] == 3:
                    for To in (1, 2):                                # a later chunk of the streamed decode: two carried frames, pt = 0
                        for resid in (0, 1):
                            add(Cin, N, ki, To, 16, 16, 0, resid, carried=True)
                if ki == 2:                                          # upsample3d's time_conv halves: every other output frame
                    for To in (1, 4):
                        for off in (0, 1):
                            add(Cin, N, ki, To, 16, 16, ot_mul=2, ot_off=off)
                if ki == 1:                                          # Resample's downsampling: stride (1, 2, 2), padding 0
                    for To in (1, 2):
                        for resid in (0, 1):
                            add(Cin, N, ki, To, 40, 56, 0, resid, stride2=1)
    # the direct-gather kernel's size thresholds: M = To * Ho * Wo just below and at 4096, Ho * Wo just below and at 32 (M >= 4096 both times),
    # and the 1 x 1 x 1 shape of the VAE's shortcuts on either side
    for ki in range(4):
        for Cin in (8, 32, 64, 96):
            for N in (32, 40, 96, 128, 384):
                for resid in (0, 1):
                    for To, H, W in ((1, 64, 64), (1, 63, 65), (128, 4, 8), (147, 4, 7), (81, 12, 16), (8, 12, 16), (17, 16, 16)):
                        add(Cin, N, ki, To, H, W, 0, resid)
                for To, H, W in ((81, 12, 16), (17, 16, 16)):        # ... and its ldc % 8 == 0 at a size it takes
                    for dldc in (4, 8):
                        add(Cin, N, ki, To, H, W, dldc=dldc)
    return rows


def geom_of(r):
    Cin, N, ki, Ti, To, H, W, pt, ups, resid, ldc, stride2, ot_mul, ot_off = r
    kt, kh, kw = KERNELS[ki]
    Ho, Wo = (2 * H, 2 * W) if ups else (H // 2, W // 2) if stride2 else (H, W)
    s, ph, pw = (2, 0, 0) if stride2 else (1, kh // 2, kw // 2)
    kpad = (kt * kh * kw * Cin + 63) // 64 * 64
    return (Ti, H, W, Cin, To, Ho, Wo, kt, kh, kw, 1, s, s, pt, ph, pw, ups, ot_mul, ot_off, N, kpad)


def write(path, classes, corrected, answers):
    """the table: one 6-character string per grid() row -- the three scail_conv3d_kernel_for answers, then the class (a hex digit, index into
    "classes") of the plain, conv + norm and next-norm form -- 60 rows to a line; "corrected": [row, form, class the old helper gave]"""
    rows = ["".join(answers[i:i + 60]) for i in range(0, len(answers), 60)]
    corr = [json.dumps(corrected[i:i + 40], separators=(",", ":"))[1:-1] for i in range(0, len(corrected), 40)]
    with open(path, "w") as f:
        f.write('{"grid": "tools/conv_dispatch_table.py grid()", "rows": %d, "classes": %s,\n "corrected": [\n%s\n],\n "answers": [\n%s\n]}\n' %
                (len(answers), json.dumps(classes), ",\n".join(corr), ",\n".join(json.dumps(r) for r in rows)))


def read(path):
    """-> (classes, corrected, [[k0, k1, k2, plain, norm, dual] per row])"""
    t = json.load(open(path))
    flat = "".join(t["answers"])
    assert len(flat) == 6 * t["rows"]
    return t["classes"], t["corrected"], [[int(c, 16) for c in flat[i:i + 6]] for i in range(0, len(flat), 6)]


def record(path):
    from scail_amd import build
    build.build(verbose=False)
    from scail_amd import lib as L
    import vae_stream_dispatch as D
    lib = L.load()
    names, out = [], []

    def idx(c):
        c = None if c is None else ":".join(str(v) for v in c)
        if c not in names:
            names.append(c)
        return "%x" % names.index(c)

    for r in grid():
        Cin, N, ki, Ti, To, H, W, pt, ups, resid, ldc, stride2, ot_mul, ot_off = r
        g = C.cast((C.c_int32 * 21)(*geom_of(r)), C.c_void_p)
        ks = [lib.scail_conv3d_kernel_for(g, ldc, N if resid else 0, m) for m in (0, 1, 2)]
        cls = [None, None, None]
        if not stride2:                         # (the old helper has no stride argument, and no ldc: it answers for ldc = N)
            kw = dict(resid=bool(resid), ups=bool(ups), ot_mul=ot_mul, ot_off=ot_off)
            cls = [D._conv(lib, Cin, N, KERNELS[ki], Ti, To, H, W, pt, fuse=f, **kw) for f in (None, "norm", "dual")]
            if resid:
                cls[1] = None                   # scail_conv3d_cl_norm takes no residual
        out.append("".join(str(k) for k in ks) + "".join(idx(c) for c in cls))
    write(path, names, [], out)
    print(f"{len(out)} rows, {len(names)} classes -> {path}")


def correct(path):
    """rewrite the rows whose class differs from the library's own answer (tests/test_conv_dispatch_cpu.py classes_of)"""
    import test_conv_dispatch_cpu as T
    classes, corrected, rows = read(path)
    lib = T.library()
    n0 = len(corrected)
    for i, (r, a) in enumerate(zip(grid(), rows)):
        for form, c in enumerate(T.classes_of(lib, r)):
            if c is None:
                continue
            if c not in classes:
                classes.append(c)
            if classes[a[3 + form]] != c:
                corrected.append([i, form, a[3 + form]])
                a[3 + form] = classes.index(c)
    assert len(classes) <= 16
    write(path, classes, corrected, ["".join("%x" % v for v in a) for a in rows])
    print(f"{len(corrected) - n0} corrections -> {path}")


if __name__ == "__main__":
    if sys.argv[1] == "--correct":
        correct(sys.argv[2])
    else:
        record(sys.argv[1])
