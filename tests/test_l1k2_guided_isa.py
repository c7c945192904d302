"""The register and LDS budget of l1k2_guided_kernel, read from the resource summary of the gfx950 code the
Makefile's flags produce: two workgroups of 256 threads per CU, that is two waves per SIMD, need at most 256
registers per lane and at most half of the CU's 160 KB of LDS each; the kernel is written for 56320 bytes and no
scratch.  No GPU is needed: the file is only compiled."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectavi_amd", "csrc")
LDS_BYTES = 32768 + 2 * 8192 + 2 * 1024 + 2 * 2048 + 4 * 256   # query rows, two tiles, their keypoints, top-2 keys, queues


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


def _compile(tmp_path_factory, source):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("isa") / (source + ".s")
    subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, source),
                                                 "-o", str(out)], check=True, cwd=CSRC)
    return out.read_text()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return _compile(tmp_path_factory, "l1k2_guided.hip")


@pytest.fixture(scope="module")
def asm_batch(tmp_path_factory):
    """l1k2_batch.hip, which holds the finish kernel of both many-pairs forms."""
    return _compile(tmp_path_factory, "l1k2_batch.hip")


def _metadata(asm, kernel):
    """The .amdhsa metadata entry of the kernel as {key: int}."""
    entries = asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:")
    mine = [e for e in entries if re.search(r"\.name:\s+\S*%s" % kernel, e)]
    assert len(mine) == 1, "expected one metadata entry for %s, found %d" % (kernel, len(mine))
    return {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", mine[0], re.M)}


def test_main_kernel_budget(asm):
    md = _metadata(asm, "l1k2_guided_kernel")
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert md["group_segment_fixed_size"] == LDS_BYTES == 56320, md
    assert 2 * md["group_segment_fixed_size"] <= 160 * 1024, md


@pytest.mark.parametrize("kernel", ["l1k2_finish_kernel", "epipolar_lines_kernel"])
def test_helper_kernels_use_no_scratch(request, kernel):
    md = _metadata(request.getfixturevalue("asm_batch" if kernel == "l1k2_finish_kernel" else "asm"), kernel)
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    assert md["group_segment_fixed_size"] == 0, md
