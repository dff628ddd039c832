"""The committed generated assembly (scail_amd/csrc/*.s) is what its generator emits today: every code object of
scail_amd/asmgen/codeobj.py CODE_OBJECTS that is committed.  (build.py would otherwise rewrite a stale file quietly.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scail_amd.asmgen import codeobj  # noqa: E402


@pytest.mark.parametrize("co", [c for c in codeobj.CODE_OBJECTS if c.committed], ids=lambda c: c.stem)
def test_generated_file_is_current(co):
    assert open(co.path("")).read() == co.text(), f"run `python -m scail_amd.asmgen.{co.gen}`"
