"""Which kernel instantiations of the library ran.

  --list     (no GPU needed) the kernel instantiations in the gfx950 code objects of the built
             libspectavi.so: the .hip_fatbin section is cut into its offload bundles, each gfx950
             code object is unbundled with clang-offload-bundler and its function symbols are read,
             demangled, with llvm-readelf.  Grouped by the source file that defines each kernel.
  --trace D  the same list diffed against the kernel names in the rocprofv3 --kernel-trace CSVs under
             D (every process's file: children traced with their parent count), names shortened as
             tools/pmc_kernels.py does: what ran, and what never ran.

    python tools/kernel_coverage.py --list
    rocprofv3 --kernel-trace --output-format csv -d D -- python -m pytest tests/test_l1k2_gpu.py ... -m gpu
    python tools/kernel_coverage.py --trace D [--files l1k2.hip,cascade.hip] [--strict]
"""
import argparse
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "spectavi_amd", "csrc")
sys.path.insert(0, HERE)
from pmc_kernels import short  # noqa: E402

BUNDLE_MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")

# Instantiations that no test can reach on purpose, printed beside the diff.
NOTES = {
    "cascade_kernels.h": [
        "the projection and scan kernels cascade.hip and cascade_batch.hip share: both files compile their own copies of "
        "the query-side instantiations, which show here once.",
    ],
    "cascade.hip": [
        "probe_table_kernel<1, 8, 7, false, false> also serves the non-shift probe of power-of-two widths "
        "for images of 4 GiB and more (xrows * dim >= 2^32); that path is not exercised by any test "
        "(the instantiation itself runs at dims 48..112).",
        "project_kernel<4, 2, true, 16> can never be selected: G = 16 needs g > 4, and g <= m <= 4 at MC 4.",
        "probe_refine_kernel<1, 2> is reached only with SPECTAVI_CASCADE_RU=2 (tests/test_knobs_gpu.py runs it in a "
        "child process); every other instantiation is one the default selection takes for some shape "
        "(spv_cascade_plan says which; tests/test_abi.py sweeps it without a GPU).",
    ],
    "ann.hip": [
        "ann_coarse_kernel<16, *> is reached only with SPECTAVI_ANN_MFMA=16, which is read once per process: "
        "tests/test_knobs_gpu.py runs the five widths in a child process (setting ann_mfma16) whose plan "
        "assertion names the shape; they show here only if the trace followed that child.",
    ],
}


def rocm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if not p:
        sys.exit("kernel_coverage: %s not found (ROCm llvm/bin)" % name)
    return p


def norm(name):
    return re.sub(r"\s+", "", short(name))


def kernel_sources():
    """kernel base name -> the .hip file, or the shared header, that defines it (`__global__ ... void NAME(`)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        text = open(path).read()
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text):
            out[m.group(1)] = os.path.basename(path)
    return out


def code_object_kernels(lib, arch):
    """Demangled kernel symbols of every `arch` code object bundled in `lib`."""
    objcopy, bundler, readelf = rocm_tool("llvm-objcopy"), rocm_tool("clang-offload-bundler"), rocm_tool("llvm-readelf")
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([objcopy, "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        data = open(fat, "rb").read()
        starts = sorted(m.start() for magic in BUNDLE_MAGICS for m in re.finditer(re.escape(magic), data))
        if not starts:
            sys.exit("kernel_coverage: no offload bundle in the .hip_fatbin section of %s" % lib)
        for i, s in enumerate(starts):
            b = os.path.join(tmp, "b%d" % i)
            with open(b, "wb") as f:
                f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            targets = subprocess.run([bundler, "--list", "--type=o", "--input=" + b], check=True,
                                     stdout=subprocess.PIPE, text=True).stdout.split()
            for t in targets:
                if not t.startswith("hip") or arch not in t:
                    continue
                co = os.path.join(tmp, "b%d.co" % i)
                subprocess.run([bundler, "--unbundle", "--type=o", "--targets=" + t, "--input=" + b,
                                "--output=" + co], check=True)
                syms = subprocess.run([readelf, "-s", "--wide", "--demangle", co], check=True,
                                      stdout=subprocess.PIPE, text=True).stdout
                for line in syms.splitlines():
                    f = line.split(None, 7)
                    if len(f) == 8 and f[3] == "FUNC" and f[4] == "GLOBAL":
                        names.add(f[7])
    return names


def instantiations(lib, arch):
    """source file -> {short name} for every kernel instantiation in the library."""
    src = kernel_sources()
    per = defaultdict(set)
    for full in code_object_kernels(lib, arch):
        s = short(full)
        per[src.get(s.split("<")[0], "?")].add(s)
    return per


def traced(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("kernel_coverage: no *kernel_trace.csv under %s" % trace_dir)
    counts = defaultdict(int)
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                counts[norm(row.get("Kernel_Name", ""))] += 1
    return counts, len(files)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "spectavi_amd", "libspectavi.so"))
    ap.add_argument("--arch", default="gfx950")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--list", action="store_true", help="list the instantiations (no GPU needed)")
    g.add_argument("--trace", metavar="DIR", help="rocprofv3 --kernel-trace --output-format csv output directory")
    ap.add_argument("--files", default="l1k2.hip,bruteforce.hip,cascade.hip,cascade_kernels.h,cascade_batch.hip,sift.hip,rectify_batch.hip,stereo_batch.hip,normalize_batch.hip,tracks_batch.hip,tracks_triangulate.hip,resect_batch.hip,bundle_adjust.hip",
                    help="source files to report (comma separated; 'all' for every file)")
    ap.add_argument("--strict", action="store_true", help="exit 1 if an instantiation never ran")
    a = ap.parse_args()

    per = instantiations(a.lib, a.arch)
    files = sorted(per) if a.files == "all" else a.files.split(",")
    if a.list:
        for f in files:
            print("%s: %d kernel instantiations" % (f, len(per.get(f, ()))))
            for k in sorted(per.get(f, ())):
                print("  " + k)
        return 0
    counts, nfiles = traced(a.trace)
    print("%d kernel trace file(s), %d dispatches" % (nfiles, sum(counts.values())))
    missing = 0
    for f in files:
        kern = sorted(per.get(f, ()))
        ran = [k for k in kern if counts.get(norm(k))]
        never = [k for k in kern if not counts.get(norm(k))]
        missing += len(never)
        print("\n%s: %d of %d instantiations ran" % (f, len(ran), len(kern)))
        for k in ran:
            print("  ran    %7d  %s" % (counts[norm(k)], k))
        for k in never:
            print("  NEVER           %s" % k)
        for n in NOTES.get(f, ()):
            print("  note: " + n)
    return 1 if a.strict and missing else 0


if __name__ == "__main__":
    sys.exit(main())
