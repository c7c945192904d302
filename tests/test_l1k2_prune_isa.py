"""The register, LDS and wait budget of l1k2_prune_kernel, read from the gfx950 assembly the Makefile's
flags produce.  The kernel's header comment asks for this check after every change; here it is mechanical.
No GPU is needed: the file is only compiled."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectavi_amd", "csrc")
KERNEL = "l1k2_prune_kernel"
MFMA = "v_mfma_i32_32x32x32_i8"


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def _makefile_flags():
    """CXXFLAGS of spectavi_amd/csrc/Makefile with $(ARCH) filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS := (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("isa") / "l1k2_prune.s"
    subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "l1k2_prune.hip"),
                                                 "-o", str(out)], check=True, cwd=CSRC)
    return out.read_text()


def _metadata(asm, kernel=KERNEL):
    """The .amdhsa metadata entry of the kernel as {key: int}."""
    entries = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")
    mine = [e for e in entries if re.search(r"\.name:\s+\S*%s" % kernel, e)]
    assert len(mine) == 1, "expected one metadata entry for %s, found %d" % (kernel, len(mine))
    return {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", mine[0], re.M)}


def _body(asm, kernel=KERNEL):
    """The instructions of the kernel, comments stripped."""
    start = re.search(r"^_Z\w*%s\w*:" % kernel, asm, re.M)
    assert start, "no label for %s" % kernel
    end = asm.index(".end_amdhsa_kernel", start.end())
    lines = [l.split(";")[0].strip() for l in asm[start.end():end].splitlines()]
    return [l for l in lines if l and not l.startswith(".")]


def _longest_mfma_run(body):
    """(index of the first, index of the last, count) of the longest run of MFMAs in `body`.  A run ends at a branch,
    a barrier or the program's end (labels are dropped by _body, so runs are told apart by the branches between them)."""
    runs, cur = [], None
    for i, l in enumerate(body):
        if l.startswith(MFMA):
            if cur is None:
                cur = [i, i, 0]
            cur[1] = i
            cur[2] += 1
        elif cur is not None and re.match(r"s_(c?branch|barrier|endpgm|setpc)", l):
            runs.append(cur)
            cur = None
    if cur is not None:
        runs.append(cur)
    assert runs, "no %s in the kernel" % MFMA
    return tuple(max(runs, key=lambda r: r[2]))


def _register_blind(lines):
    """The lines with every register operand (v12, s[4:5], a3: single registers and ranges) replaced by one placeholder."""
    return [re.sub(r"\b[vsa](\d+|\[\d+:\d+\])", "R", l) for l in lines]


def test_register_and_lds_budget(asm):
    md = _metadata(asm)
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert md["group_segment_fixed_size"] <= 81920, md


def test_no_vector_memory_wait_inside_a_tiles_mfmas(asm):
    """In the longest run of MFMAs (the 32 of a tile) no s_waitcnt between the first and the last names vmcnt."""
    body = _body(asm)
    first, last, count = _longest_mfma_run(body)
    assert count == 32, "the tile's MFMA run has %d instructions, expected 32" % count
    waits = [l for l in body[first:last + 1] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert not waits, "%d vmcnt waits inside the tile's MFMA run: %s" % (len(waits), waits)
