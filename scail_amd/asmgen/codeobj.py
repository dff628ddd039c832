"""The code-object text every generator shares -- kernel descriptor (.amdhsa_kernel), metadata (.amdgpu_metadata), file layout -- and
the table of the code objects made from the generators (CODE_OBJECTS), which scail_amd/build.py, ``python -m scail_amd.asmgen.<gen>``
and the tests read.

A generator describes each kernel by the few values that differ between kernels (``Kernel``) and renders a file with
``assembly(HEAD, kernels)``."""
from __future__ import annotations

import importlib
import os
import sys
from dataclasses import dataclass
from typing import Iterable, Tuple

ASMGEN = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(ASMGEN), "csrc")


@dataclass(frozen=True)
class Kernel:
    name: str
    comment: str           # header comment: "// ---- kernel <name>: <comment> ----"
    body: str              # the rendered program (isa.render)
    lds_bytes: int
    kernarg_size: int
    vgprs: int = 512       # arch + accumulation registers per lane
    agprs: int = 256       # accumulation registers (the top of the file: accum_offset = vgprs - agprs)
    sgprs: int = 96        # next_free_sgpr
    wg_size: int = 256     # max_flat_workgroup_size


def kernel_text(k: Kernel) -> str:
    return f"""// ---- kernel {k.name}: {k.comment} ----
\t.text
\t.protected\t{k.name}
\t.globl\t{k.name}
\t.p2align\t8
\t.type\t{k.name},@function
{k.body}.L{k.name}_end:
\t.size\t{k.name}, .L{k.name}_end-{k.name}
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {k.name}
\t\t.amdhsa_group_segment_fixed_size {k.lds_bytes}
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_kernarg_size {k.kernarg_size}
\t\t.amdhsa_user_sgpr_count 2
\t\t.amdhsa_user_sgpr_kernarg_segment_ptr 1
\t\t.amdhsa_system_sgpr_workgroup_id_x 1
\t\t.amdhsa_system_sgpr_workgroup_id_y 1
\t\t.amdhsa_system_sgpr_workgroup_id_z 1
\t\t.amdhsa_system_vgpr_workitem_id 0
\t\t.amdhsa_next_free_vgpr {k.vgprs}
\t\t.amdhsa_next_free_sgpr {k.sgprs}
\t\t.amdhsa_accum_offset {k.vgprs - k.agprs}
\t\t.amdhsa_reserve_vcc 1
\t\t.amdhsa_float_round_mode_32 0
\t\t.amdhsa_float_round_mode_16_64 0
\t\t.amdhsa_float_denorm_mode_32 3
\t\t.amdhsa_float_denorm_mode_16_64 3
\t\t.amdhsa_dx10_clamp 1
\t\t.amdhsa_ieee_mode 1
\t.end_amdhsa_kernel
"""


def metadata(kernels) -> str:
    ks = "".join(f"""  - .agpr_count:     {k.agprs}
    .args:
      - .offset:         0
        .size:           {k.kernarg_size}
        .value_kind:     by_value
    .group_segment_fixed_size: {k.lds_bytes}
    .kernarg_segment_align: 8
    .kernarg_segment_size: {k.kernarg_size}
    .max_flat_workgroup_size: {k.wg_size}
    .name:           {k.name}
    .private_segment_fixed_size: 0
    .sgpr_count:     102
    .sgpr_spill_count: 0
    .symbol:         {k.name}.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     {k.vgprs}
    .vgpr_spill_count: 0
    .wavefront_size: 64
""" for k in kernels)
    return f"""\t.amdgpu_metadata
---
amdhsa.kernels:
{ks}amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
\t.end_amdgpu_metadata
"""


def assembly(head: str, kernels: Iterable[Kernel]) -> str:
    """One .s file: the generator's header comment, the target, every kernel with its descriptor, then the metadata of all of them."""
    kernels = list(kernels)
    return (head + "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.amdhsa_code_object_version 6\n" +
            "".join(kernel_text(k) for k in kernels) + metadata(kernels))


@dataclass(frozen=True)
class CodeObject:
    stem: str                  # <stem>.s -> <stem>.hsaco, embedded by csrc/*.hip from <stem>_hsaco.inc
    gen: str                   # generator module in this package
    lists: Tuple[str, ...]     # the generator's config lists the code object holds, in order
    variants: bool = True      # the measurement build adds the generator's variant_cfgs()
    committed: bool = True     # csrc/<stem>.s is committed (tests/test_codeobj_cpu.py selects by it); False: the assembly is a build product,
                               # written to the build directory by scail_amd/build.py -- the generator is its only source

    def module(self):
        return importlib.import_module(f"{__package__}.{self.gen}")

    def cfgs(self, variants: bool = False) -> list:
        m = self.module()
        return [c for n in self.lists for c in getattr(m, n)] + (m.variant_cfgs() if variants and self.variants else [])

    def text(self, variants: bool = False) -> str:
        return self.module().assembly(self.cfgs(variants))

    def path(self, objdir: str = "") -> str:
        """csrc/<stem>.s of a committed code object; <objdir>/<stem>.s (the build directory) otherwise"""
        return os.path.join(CSRC if self.committed else (objdir or os.path.join(os.path.dirname(os.path.dirname(ASMGEN)), "build")), self.stem + ".s")


CODE_OBJECTS = [
    CodeObject("attn4", "attn4", ("SHIPPED",)),
    CodeObject("attn4v", "attn4", ("VROWS",), variants=False, committed=False),      # 0.6 MB of text nobody reads: generated at build time
    CodeObject("gemm4", "gemm4", ("DEFAULTS",)),
    CodeObject("conv4", "conv4", ("DEFAULTS",)),
    CodeObject("conv4u", "conv4", ("UPSAMPLE", "NARROW", "FUSED", "CONT", "RESNORM"), variants=False),
]


def write_if_changed(path: str, text: str) -> None:
    if not os.path.exists(path) or open(path).read() != text:
        open(path, "w").write(text)


def main(gen: str) -> None:
    """``python -m scail_amd.asmgen.<gen> [--check] [--variants DIR]``: rewrite the generator's code objects where stale; --check: exit 1
    if any of them differs from the generator instead; --variants DIR: write the measurement build's <stem>_variants.s into DIR."""
    cos = [c for c in CODE_OBJECTS if c.gen == gen and (c.committed or "--variants" in sys.argv)]
    if "--variants" in sys.argv:
        dst = sys.argv[sys.argv.index("--variants") + 1]
        for c in cos:
            out = os.path.join(dst, c.stem + "_variants.s")
            open(out, "w").write(c.text(variants=True))
            print(out)
        return
    if "--check" in sys.argv:
        sys.exit(0 if all(os.path.exists(c.path()) and open(c.path()).read() == c.text() for c in cos) else 1)
    for c in cos:
        text = c.text()
        write_if_changed(c.path(), text)
        print(c.path(), len(text.splitlines()), "lines")
