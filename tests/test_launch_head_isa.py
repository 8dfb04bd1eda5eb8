"""dec_linear_kernel's launch head in the gfx950 device assembly (CPU check, no GPU).

The kernel takes what its first loads need as leading scalar parameters and declin.hip is compiled with the kernarg
preload (csrc/Makefile), so those values are in SGPRs at wave start and the first weight load is issued without a
trip to the argument buffer.  For every instantiation of dec_linear_kernel this holds the two properties the source
cannot show: a non-zero ``.amdhsa_user_sgpr_kernarg_preload_length``, and at most one ``s_waitcnt lgkmcnt`` between
the kernel's entry (behind the compatibility prologue for firmware that does not preload, which ends at the 256-byte
alignment) and its first vector memory load.  The parent of this file's change had four such waits there
(profiles/r10_launch_head.txt).  The assembly is obtained as tools/isa_scan.py does, with the Makefile's per-file flags.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_scan  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_scan.HIPCC) and not shutil.which("hipcc"),
                                reason="hipcc not available")

# the instantiations choose() gives the greedy step's plan at large-v3 (d 1280, ffn 5120, B = 32): o / xo (16-row
# chunks), fc1 (LayerNorm, bf16 C, two column blocks), fc2 (K split)
GREEDY = [r"dec_linear_kernelILi5ELi1ELb0ELi1EfLb0EE", r"dec_linear_kernelILi5ELi2ELb1ELi0EtLb1EE",
          r"dec_linear_kernelILi5ELi1ELb0ELi1EfLb1EE"]
_VMEM = re.compile(r"^(global|buffer|flat)_(load|store|atomic)")


def makefile_flags(obj: str) -> list[str]:
    """The flags csrc/Makefile adds for one object file (``$(BUILD)/<obj>: CXXFLAGS += ...``), variables expanded."""
    with open(os.path.join(isa_scan.CSRC, "Makefile")) as f:
        text = f.read()
    var = dict(re.findall(r"^(\w+)\s*\?=\s*(\S+)\s*$", text, re.M))
    m = re.search(r"^[^\n#]*\$\(BUILD\)/" + re.escape(obj) + r"[^\n:]*:\s*CXXFLAGS\s*\+=\s*(.+)$", text, re.M)
    assert m, f"csrc/Makefile has no per-file flags for {obj}"
    return re.sub(r"\$\((\w+)\)", lambda v: var[v.group(1)], m.group(1)).split()


@pytest.fixture(scope="module")
def asm():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([isa_scan.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                        *makefile_flags("declin.o"), "--cuda-device-only", "-S", "-o", out,
                        os.path.join(isa_scan.CSRC, "declin.hip")], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def preload_lengths(asm: str) -> dict[str, int]:
    return {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel (\S+).*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", asm, re.S)}


def head_waits(body: list[str]) -> int:
    """``s_waitcnt lgkmcnt`` between the kernel's entry proper and its first vector memory instruction."""
    start = next((i for i, t in enumerate(body) if t.startswith(".p2align")), -1) + 1  # (behind the prologue)
    n = 0
    for t in body[start:]:
        if _VMEM.match(t):
            return n
        if t.startswith("s_waitcnt") and "lgkmcnt" in t:
            n += 1
    raise AssertionError("no vector memory instruction")


def test_makefile_preloads_declin():
    assert any("amdgpu-kernarg-preload-count=" in f for f in makefile_flags("declin.o"))


def test_every_dec_linear_kernel_preloads_its_head(asm):
    lens = {k: v for k, v in preload_lengths(asm).items() if "dec_linear_kernel" in k}
    assert len(lens) >= 3 and all(re.search(p, "\n".join(lens)) for p in GREEDY), sorted(lens)
    # W, x and xz (two dwords each), K / 32, xt, the K splits, the waves, the multiplier: 11 dwords; fewer means a head
    # value went back into the struct or the option no longer reaches this file
    assert all(v >= 11 for v in lens.values()), {k: v for k, v in lens.items() if v < 11}


def test_first_load_waits_for_at_most_one_scalar_trip(asm):
    ks = {k: b for k, b in isa_scan.kernels(asm).items() if "dec_linear_kernel" in k}
    assert len(ks) >= 3
    waits = {k: head_waits(b) for k, b in ks.items()}
    print("dec_linear_kernel: s_waitcnt lgkmcnt before the first vector memory instruction:", sorted(set(waits.values())))
    assert all(n <= 1 for n in waits.values()), {k: n for k, n in waits.items() if n > 1}
    for p in GREEDY:  # the greedy step's three: none at all
        name, body = isa_scan.find(asm, p)
        assert head_waits(body) == 0, name
