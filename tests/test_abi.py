"""CPU-only: the C-ABI library loads, exports every symbol include/*.h declares, and the
front-end's argument validation mirrors the reference's.  No compute calls (no GPU here)."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": ct.c_int, "int32_t": ct.c_int32, "uint32_t": ct.c_uint32, "long long": ct.c_longlong,
           "unsigned long long": ct.c_ulonglong, "size_t": ct.c_size_t, "float": ct.c_float, "double": ct.c_double,
           "bool": ct.c_bool}
POINTEES = dict(SCALARS, int8_t=ct.c_int8, uint8_t=ct.c_uint8, uint64_t=ct.c_uint64)
C_CONTIGUOUS = 0x1   # NPY_ARRAY_C_CONTIGUOUS, as numpy.ctypeslib.ndpointer keeps it in _flags_


def c_type(text, named):
    """A return type or a parameter as the headers spell them -> (base type, pointer depth):
    'const double *P0' -> ('double', 1), 'int out[5]' -> ('int', 1), 'const float *const *d_x' -> ('float', 2)."""
    text, dims = re.subn(r"\[\d+\]", "", text)
    words = [w for w in text.replace("*", " ").split() if w != "const"]
    base = " ".join(words[:-1] if named else words)
    assert base in POINTEES or base in ("void", "char", "NdArray"), "unknown C type in %r" % text
    return base, text.count("*") + (1 if dims else 0)


def declared_prototypes():
    """{name: ((base, depth) of the return type, [(base, depth) of every parameter])} of every function
    the two headers declare.  Understands the spellings they use and fails on any other."""
    protos = {}
    for hdr in ("spectavi_amd.h", "NdArray.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        assert "//" not in text and "\\\n" not in text
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
        text = re.sub(r"typedef struct NdArray \{.*?\} NdArray;", "", text, flags=re.S)
        text = text.replace('extern "C" {', "")
        for decl in text.split(";"):
            decl = " ".join(decl.split())
            if decl in ("", "}"):   # "}" closes extern "C"
                continue
            m = re.fullmatch(r"(.*?)(\w+) ?\((.*)\)", decl)
            assert m and m.group(2) not in protos, "cannot parse %r" % decl
            params = [] if m.group(3) == "void" else [c_type(a, True) for a in m.group(3).split(",")]
            protos[m.group(2)] = (c_type(m.group(1), False), params)
    return protos


def declared_symbols():
    return sorted(declared_prototypes())


def accepts(ctype, base, depth):
    """Whether a ctypes restype / argtypes entry can stand for the C type (base, depth)."""
    from spectavi_amd.ndarray import NdArray
    if depth == 0:
        return ctype is (None if base == "void" else SCALARS[base])
    if depth == 2:
        return ctype is ct.POINTER(ct.c_void_p)
    if base in ("void", "char", "NdArray"):
        return ctype is {"void": ct.c_void_p, "char": ct.c_char_p, "NdArray": ct.POINTER(NdArray)}[base]
    if ctype is ct.c_void_p or ctype is ct.POINTER(POINTEES[base]):
        return True
    return (hasattr(ctype, "_dtype_") and ctype._dtype_ == np.dtype(POINTEES[base])   # an ndpointer class
            and bool((ctype._flags_ or 0) & C_CONTIGUOUS))


def mismatches(proto, decl):
    """What is wrong with the ctypes prototype (restype, [argtypes]) of a function declared as decl."""
    (restype, argtypes), (ret, params) = proto, decl
    if len(argtypes) != len(params):
        return ["%d arguments, the header has %d" % (len(argtypes), len(params))]
    bad = [] if accepts(restype, *ret) else ["restype %r for %s" % (restype, ret)]
    return bad + ["slot %d: %r for %s" % (k, a, c) for k, (a, c) in enumerate(zip(argtypes, params))
                  if not accepts(a, *c)]


def test_prototype_table_names_every_declared_function():
    from spectavi_amd._proto import PROTOTYPES
    assert set(PROTOTYPES) == set(declared_prototypes()), set(PROTOTYPES) ^ set(declared_prototypes())


def test_prototype_table_agrees_with_the_headers():
    """Every restype and every argtypes slot of spectavi_amd/_proto.py against include/*.h."""
    from spectavi_amd._proto import PROTOTYPES
    decls = declared_prototypes()
    wrong = {n: mismatches(PROTOTYPES[n], d) for n, d in decls.items() if mismatches(PROTOTYPES[n], d)}
    assert not wrong, wrong


def test_prototype_check_refuses_wrong_prototypes():
    from numpy.ctypeslib import ndpointer
    i, f64a = ct.c_int, ndpointer(np.float64, flags="C_CONTIGUOUS")
    decls = declared_prototypes()
    for name, proto in (
            ("spv_set_device", (i, [])),                                        # one argument too few
            ("spv_shard_lo", (ct.c_longlong, [i, i, i])),                       # c_int for a long long
            ("spv_l1k2_workspace_bytes", (i, [i, i, i])),                       # c_int for a size_t return
            ("spv_rectify_shape", (i, [i, i, i, ct.c_float, ct.POINTER(i)])),   # c_float for a double
            ("spv_rectify_fundamental", (i, [ndpointer(np.float32, flags="C_CONTIGUOUS"), f64a, f64a])),
            ("spv_rectify_fundamental", (i, [ndpointer(np.float64), f64a, f64a])),   # contiguity not required
            ("spv_profile_enable", (None, [ct.c_void_p])),                      # c_void_p for an int
            ("spv_last_error", (ct.c_void_p, [])),                              # not a string
            ("spv_l1k2_gathered_device", (i, [i, ct.POINTER(i)] + [ct.c_void_p] * 2 + [i, ct.c_longlong, i]
                                          + [ct.c_void_p] * 2 + [i]))):         # c_void_p for a T *const *
        assert mismatches(proto, decls[name]), name


def test_library_carries_the_table_after_importing_the_loader_alone():
    """In a fresh process, so that nothing imported earlier in this session can have typed clib."""
    import subprocess
    import sys
    code = ("import sys; from spectavi_amd._lib import clib; from spectavi_amd._proto import PROTOTYPES\n"
            "assert not {'torch', 'spectavi_amd.feature', 'spectavi_amd.mvg', 'spectavi_amd.device'} & set(sys.modules)\n"
            "for n, (r, a) in PROTOTYPES.items():\n"
            "    fn = getattr(clib, n)\n"
            "    assert fn.restype is r and len(fn.argtypes) == len(a) and all(x is y for x, y in zip(fn.argtypes, a)), n\n"
            "print('typed', len(PROTOTYPES))")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("typed"), r.stdout + r.stderr


def test_library_exports_every_declared_symbol():
    from spectavi_amd._lib import clib
    names = declared_symbols()
    assert {"nn_bruteforcel1k2", "nn_cascading_hash", "dlt_triangulate", "dlt_reprojection_error",
            "spv_l1k2_device", "spv_cascade_device", "spv_dlt_triangulate_device",
            "ndarray_set_size", "ndarray_alloc"} <= set(names)
    for n in names:
        assert hasattr(clib, n), "libspectavi.so does not export %s" % n


def test_ndarray_struct_matches_header():
    from spectavi_amd._lib import clib
    from spectavi_amd.ndarray import NdArray
    assert ct.sizeof(NdArray) == 8 + 4 * 8 + 4 + 4
    a = NdArray(dtype='int32')
    clib.ndarray_set_size(ct.byref(a), 3, 2)
    assert clib.ndarray_alloc(ct.byref(a)) == 0
    ct.memmove(a.m_data, (ct.c_int32 * 6)(1, 2, 3, 4, 5, 6), 24)
    arr = a.asarray()
    assert arr.dtype == np.int32 and arr.shape == (3, 2) and arr.tolist() == [[1, 2], [3, 4], [5, 6]]


def test_status_api_without_gpu():
    from spectavi_amd import _lib
    assert _lib.clib.spv_version().startswith(b"spectavi_amd")
    assert _lib.device_count() >= 0
    # invalid arguments are rejected before any device work
    from spectavi_amd import feature
    st = feature._spv_generate_hash_dict(1, 0, 4, 2, np.zeros(1, np.float32))
    assert st == _lib.SPV_ERR_INVALID
    with pytest.raises(_lib.SpectaviError):
        _lib.check(st)


def test_hash_dict_is_mt19937_normal_stream():
    from spectavi_amd import feature
    d = feature.generate_hash_dict(123, 16, 5, 3)
    assert d.shape == (3, 16, 5) and d.dtype == np.float32
    d2 = feature.generate_hash_dict(123, 16, 5, 3)
    assert np.array_equal(d, d2)
    assert not np.array_equal(d, feature.generate_hash_dict(124, 16, 5, 3))
    big = feature.generate_hash_dict(7, 128, 17, 2)
    assert abs(float(big.mean())) < 0.05 and abs(float(big.std()) - 1) < 0.05


def test_frontend_validation_matches_reference():
    from spectavi_amd import feature, mvg
    with pytest.raises(AssertionError):  # reference feature.py:297-299
        feature.nn_bruteforcel1k2(np.zeros((4, 16), np.uint8), np.zeros((4, 32), np.uint8))
    with pytest.raises(ValueError):      # reference throws runtime_error (BruteForceNnL1K2.h:77-81)
        feature.nn_bruteforcel1k2(np.zeros((4, 24), np.uint8), np.zeros((4, 24), np.uint8))
    P = np.zeros((3, 4))
    with pytest.raises(TypeError):       # reference mvg.py:283-294
        mvg.dlt_triangulate(np.zeros((4, 4)), P, np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(TypeError):
        mvg.dlt_triangulate(P, P, np.zeros((2, 3)), np.zeros((3, 3)))
    with pytest.raises(TypeError):
        mvg.dlt_triangulate(P, P, np.zeros((2, 2)), np.zeros((2, 2)))
    assert feature.auto_hash_bit_rate(1_000_000, 1_000_000) == 17  # reference feature.py:366-367
    assert feature.auto_hash_bit_rate(200, 200) == 5 and feature.auto_hash_bit_rate(90, 90) == 3


def test_normalize_properties():
    """reference spectavi/feature.py:384-407: integer-valued, in [-128,127], zero column mean
    before scaling, width padded to a multiple of 16."""
    from spectavi_amd import feature
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 132)).astype(np.float32) * rng.uniform(0.1, 10, (1, 132))
    out = feature.normalize_to_ubyte_and_multiple_16_dim(x)
    assert out.dtype == np.float32 and out.shape == (50, 144)
    assert np.all(out == np.round(out)) and out.min() >= -128 and out.max() <= 127
    assert np.all(out[:, 132:] == 0)
    assert np.all(np.abs(out[:, :132]).max(0) >= 127)
    assert np.all(np.abs(out[:, :132].mean(0)) < 1.0)


def test_no_gpu_is_a_loud_error():
    """Without a device the product path must fail, never fall back to a CPU computation."""
    from spectavi_amd import _lib, feature
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    x = np.zeros((4, 16), np.uint8)
    with pytest.raises(_lib.SpectaviError):
        feature.nn_bruteforcel1k2(x, x)


def test_frontend_signatures_match_reference_source():
    """The hot-path front-end functions keep the reference's parameter names and defaults, and the
    ctypes argtypes lists have the reference's lengths.  The reference's side is stored in
    tests/golden/reference_frontend_signatures.json (tests/golden/make_golden.py: its source parsed
    as text with ast; nothing imported or executed from it)."""
    import inspect
    import json
    from spectavi_amd import feature, mvg

    with open(os.path.join(ROOT, "tests", "golden", "reference_frontend_signatures.json")) as f:
        ref = json.load(f)
    funs, argl = ref["functions"], ref["argtypes_len"]
    for mod, names in ((feature, ["nn_bruteforcel1k2", "nn_cascading_hash",
                                  "normalize_to_ubyte_and_multiple_16_dim"]),
                       (mvg, ["dlt_triangulate", "dlt_reprojection_error", "hnormalize",
                              "ransac_fitter", "seven_point_algorithm"])):
        mfun = funs[mod.__name__.rsplit(".", 1)[-1]]
        for name in names:
            sig = inspect.signature(getattr(mod, name))
            ours = list(sig.parameters)
            our_defaults = [p.default for p in sig.parameters.values() if p.default is not inspect._empty]
            assert ours == mfun[name]["params"], name
            assert our_defaults == mfun[name]["defaults"], name
    assert len(feature._nn_bruteforcel1k2.argtypes) == argl["feature"]["_nn_bruteforcel1k2"] == 8
    assert len(feature._nn_cascading_hash.argtypes) == argl["feature"]["_nn_cascading_hash"] == 11
    assert len(mvg._dlt_triangulate.argtypes) == argl["mvg"]["_dlt_triangulate"] == 6
    assert len(mvg._dlt_reprojection_error.argtypes) == argl["mvg"]["_dlt_reprojection_error"] == 6
    assert len(mvg._ransac_fitter.argtypes) == argl["mvg"]["_ransac_fitter"] == 14
    assert len(mvg._seven_point_algorithm.argtypes) == argl["mvg"]["_seven_point_algorithm"] == 4


def test_only_the_declared_api_is_exported():
    """libspectavi.so is built -fvisibility=hidden: its dynamic symbol table holds the declared
    extern "C" API and nothing else of its own (no C++ internals another library could interpose)."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "spectavi_amd", "libspectavi.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert exported == set(declared_symbols()), exported ^ set(declared_symbols())


def test_record_pack_and_widen_arithmetic():
    """The 16-byte (idx0, idx1, d0, d1) record that the RCCL gather moves (spectavi_amd/csrc/records.h,
    the same inline functions the device kernels call): (size_t)-1 travels as -1 and comes back as
    (size_t)-1, indices up to 2^31-1 and both distance types survive bit for bit, ragged shards map
    back to their rows.  Host functions only; no GPU involved."""
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    u64p, i32p = ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_int32)
    rng = np.random.default_rng(9)
    none = np.iinfo(np.uint64).max
    for total, G in ((1, 1), (7, 1), (7, 3), (8, 8), (1001, 3), (1000, 8), (5, 4), (64, 7)):
        idx = rng.integers(0, 2**31, (total, 2)).astype(np.uint64)
        idx[0, 0] = 2**31 - 1
        idx[rng.random(total) < 0.2, 1] = none               # one neighbour only
        idx[rng.random(total) < 0.1] = none                  # none at all
        for dist in (rng.integers(0, 2**31, (total, 2)).astype(np.int32),
                     rng.standard_normal((total, 2)).astype(np.float32)):
            dist[idx == none] = 2147483647 if dist.dtype == np.int32 else 2147483648.0
            # what each rank would pack from its contiguous shard, padded to the largest shard
            base, extra = divmod(total, G)
            max_cnt = base + (1 if extra else 0)
            rec = np.full((G, max_cnt, 4), 0x5A5A5A5A, np.int32)
            lo = 0
            for r in range(G):
                cnt = base + (1 if r < extra else 0)
                part_i = np.ascontiguousarray(idx[lo:lo + cnt])
                part_d = np.ascontiguousarray(dist[lo:lo + cnt])
                out = np.empty((cnt, 4), np.int32)
                assert clib.spv_records_pack(part_i.ctypes.data_as(u64p), part_d.ctypes.data, cnt,
                                             out.ctypes.data_as(i32p)) == 0
                assert np.array_equal(out[:, :2] == -1, part_i == none)
                assert np.array_equal(out[:, 2:].view(dist.dtype), part_d)
                rec[r, :cnt] = out
                lo += cnt
            gi, gd = np.empty((total, 2), np.uint64), np.empty((total, 2), dist.dtype)
            assert clib.spv_records_unpack(rec.ctypes.data_as(i32p), total, G, max_cnt, gi.ctypes.data_as(u64p),
                                           gd.ctypes.data) == 0
            assert np.array_equal(gi, idx) and np.array_equal(gd.view(np.uint32), dist.view(np.uint32))
    # python statement of the same record (sharded.py) agrees
    import torch
    from spectavi_amd.sharded import pack_records, unpack_records
    idx = np.array([[5, none], [none, none], [2**31 - 1, 0]], np.uint64)
    dist = np.array([[7, 2147483647], [2147483647, 2147483647], [0, 65280]], np.int32)
    rec = np.empty((3, 4), np.int32)
    clib.spv_records_pack(idx.ctypes.data_as(u64p), dist.ctypes.data, 3, rec.ctypes.data_as(i32p))
    trec = pack_records(torch.from_numpy(idx.view(np.int64)), torch.from_numpy(dist))
    assert np.array_equal(trec.numpy(), rec)
    ti, td = unpack_records(trec)
    assert np.array_equal(ti.numpy().view(np.uint64), idx) and np.array_equal(td.numpy(), dist)
    # a max_cnt smaller than the largest shard is refused
    assert clib.spv_records_unpack(rec.ctypes.data_as(i32p), 3, 2, 1, idx.ctypes.data_as(u64p),
                                   dist.ctypes.data) == SPV_ERR_INVALID


def test_gather_mode_api_without_gpu():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    assert clib.spv_set_gather_mode(7) == SPV_ERR_INVALID
    for mode in (1, 0, -1):
        assert clib.spv_set_gather_mode(mode) == 0


def test_ransac_sample_is_the_reference_draw():
    """floyd_sample (reference src/RansacFitter.h:120-132): seven distinct rows per try, values in
    [1, npt-1] (the reference's range starts at 1), reproducible per seed.  Host-only logic: runs without a GPU."""
    from spectavi_amd import mvg
    for npt in (10, 11, 50, 100000):
        s = mvg.ransac_sample(5, npt, 400)
        assert s.shape == (400, 7) and s.min() >= 1 and s.max() <= npt - 1
        assert all(len(set(r)) == 7 for r in s.tolist())
        assert np.array_equal(s, mvg.ransac_sample(5, npt, 400))
        assert not np.array_equal(s, mvg.ransac_sample(6, npt, 400))
    with pytest.raises(Exception):
        mvg.ransac_sample(1, 9, 1)


def test_ransac_fit_argument_checks_without_gpu():
    """Argument checks of the RANSAC entry points happen before any device is touched."""
    from spectavi_amd import mvg
    from spectavi_amd._lib import SPV_ERR_INVALID
    x = np.zeros((12, 3))
    ok, n = ct.c_int32(0), ct.c_int32(0)
    pct = ct.c_double(0)
    F, P, idx = np.zeros(9), np.zeros(12), np.zeros(12, np.int32)

    def call(npt, tries):
        return mvg._spv_ransac_fit(x, x, npt, .9, .5, tries, 1, 3e-2, 1, ct.byref(ok), F, P, ct.byref(pct), idx, ct.byref(n),
                                   None, None, None)
    assert call(9, 10) == SPV_ERR_INVALID        # fewer than 10 correspondences (the reference's constructor throws)
    assert call(12, -1) == SPV_ERR_INVALID
    assert call(12, 800000000) == SPV_ERR_INVALID


def test_l1k2_variant_cases_reach_every_instantiation():
    """spv_l1k2_plan (host only) on the case table of tests/test_l1k2_variants_gpu.py: every case
    gets the (width, queries per lane) it is written for, and together the cases reach exactly the
    instantiations l1k2_run launches (INSTANTIATED in tests/l1k2_variant_cases.py, kept beside the
    table `TileWidths` of l1k2.hip) and all three merge forms.  A retuned plan or a new width that
    leaves a kernel without a case fails here, without a GPU."""
    from spectavi_amd import device
    from tests import l1k2_variant_cases as lc
    reached, merges = set(), set()
    for case in lc.CASES:
        xrows, yrows, dim = case[:3]
        plan = device.l1k2_plan(xrows, yrows, dim)
        key = lc.plan_key(plan)
        assert key[:2] == case[5], (lc.case_id(case), plan)
        assert xrows % plan["slice_rows"] != 0, ("the last slice must be ragged", lc.case_id(case), plan)
        if key[1] > 1:
            assert yrows % (256 * key[1]) == 1, ("one live query in the last block", lc.case_id(case))
        reached.add(key)
        merges.add(lc.merge_form(plan))
    assert reached == lc.INSTANTIATED
    assert merges == lc.MERGE_FORMS


def test_l1k2_plan_rejects_bad_shapes():
    from spectavi_amd import _lib, device
    for args in ((10, 10, 24), (10, 10, 0), (-1, 10, 16), (10, 10, 2064)):
        with pytest.raises(_lib.SpectaviError):
            device.l1k2_plan(*args)
    assert device.l1k2_plan(0, 1, 2048) == dict(dim_pad=2048, q=1, slices=1, slice_rows=64, wide=True)


def test_cascade_variant_cases_reach_every_projection_form():
    """spv_cascade_plan (host only) on the case table of tests/test_cascade_variants_gpu.py, at that
    test's own row counts: every case gets the query-side projection instantiation it is written
    for, and together the cases reach every form the default selection can pick
    (REACHABLE_QUERY_FORMS in tests/cascade_variant_cases.py), each once.  A retuned threshold in
    cascade_plan that leaves a kernel without a case fails here, without a GPU."""
    from spectavi_amd import device
    from tests import cascade_variant_cases as cc
    for case in cc.CASES:
        dim, m, n, g, target = case
        assert dim % 16 == 0 and 1 <= m <= 31 and n >= 1 and 0 <= g <= min(m, 16)
        plan = device.cascade_plan(3000, 1100, dim, m, n, g)
        assert plan["project_query"] == target, (cc.case_id(case), plan)
        assert plan["project_db"] == cc.database_form(target), (cc.case_id(case), plan)
    targets = [c[4] for c in cc.CASES]
    assert set(targets) == cc.REACHABLE_QUERY_FORMS and len(targets) == len(set(targets))


def test_cascade_plan_names_only_shipped_kernels(monkeypatch):
    """spv_cascade_plan over a grid of shapes: every kernel it names is in the static sets of
    tests/cascade_variant_cases.py (the instantiations cascade.hip ships), and the probes named are
    all of PROBE_FORMS but the one only SPECTAVI_CASCADE_RU=2 selects -- probe_table_kernel<1, 8, 7, false, false>, which also serves power-of-two
    widths over images of 4 GiB and more, is reached at the widths that are no power of two; the
    4 GiB rule itself is asked for directly.  Bad shapes are SPV_ERR_INVALID."""
    from spectavi_amd import _lib, device
    from tests import cascade_variant_cases as cc
    for k in ("MFMA", "MFMA4", "GROUP", "QHIST", "SORT", "RU"):
        monkeypatch.delenv("SPECTAVI_CASCADE_" + k, raising=False)
    probes, queries = set(), set()
    for dim in list(range(16, 257, 16)) + [512, 1024, 2048]:
        for m in range(1, 32):
            for n in (1, 2, 3, 4, 9, 17):
                for g in sorted({0, 2, 4, 5, min(m, 16)}):
                    if g > m:
                        continue
                    for xrows, yrows in ((0, 1), (3000, 1100), (70000, 70000)):
                        plan = device.cascade_plan(xrows, yrows, dim, m, n, g)
                        assert plan["project_query"] in cc.REACHABLE_QUERY_FORMS, plan
                        assert plan["project_db"] == cc.database_form(plan["project_query"]), plan
                        assert plan["probe"] in cc.PROBE_FORMS, plan
                        assert plan["probe_kind"] == plan["probe"].startswith("probe_table"), plan
                        assert plan["sorted"] == (plan["probe"].startswith("probe_table") and n <= 8 and yrows >= 65536), plan
                        assert plan["qhist_fused"] == (plan["sorted"] and plan["family"] != 0), plan
                        probes.add(plan["probe"])
                        queries.add(plan["project_query"])
    assert probes == cc.PROBE_FORMS - cc.KNOB_PROBE_FORMS
    monkeypatch.setenv("SPECTAVI_CASCADE_RU", "2")
    assert {device.cascade_plan(3000, 1100, dim, 25, 2, 3)["probe"] for dim in (16, 128, 144)} == \
        cc.KNOB_PROBE_FORMS | {"probe_refine_kernel<2, 4>"}
    monkeypatch.delenv("SPECTAVI_CASCADE_RU")
    assert queries == cc.REACHABLE_QUERY_FORMS
    assert device.cascade_plan((1 << 25) - 1, 1, 128, 8, 2, 2)["probe"] == "probe_table_kernel<1, 8, 7, true, true>"
    assert device.cascade_plan(1 << 25, 1, 128, 8, 2, 2)["probe"] == "probe_table_kernel<1, 8, 7, false, false>"
    out = (ct.c_int * 12)(*([-7] * 12))
    for dim, m, n, g in ((24, 8, 2, 2), (128, 0, 2, 0), (128, 32, 2, 2), (128, 4, 2, 5), (128, 20, 2, 17), (2064, 8, 2, 2)):
        assert _lib.clib.spv_cascade_plan(3000, 1100, dim, m, n, g, out) == _lib.SPV_ERR_INVALID, (dim, m, n, g)
        assert _lib.clib.spv_last_error(), (dim, m, n, g)
        assert list(out) == [-7] * 12
        with pytest.raises(_lib.SpectaviError):
            device.cascade_plan(3000, 1100, dim, m, n, g)


def test_cascade_knob_settings_change_the_plan(monkeypatch):
    """What the children of tests/test_knobs_gpu.py assert before each case, without a GPU: under each
    cascade setting of tests/knob_child.py the plan of every case shows the form the knob forces."""
    from spectavi_amd import device
    from tests.knob_child import PLAN_WANTS, SETTINGS
    assert set(PLAN_WANTS) == {s for s, (_, kind, _) in SETTINGS.items() if kind == "cascade"}
    for setting, wants in PLAN_WANTS.items():
        for k in ("MFMA", "MFMA4", "GROUP", "QHIST", "SORT", "RU"):
            monkeypatch.delenv("SPECTAVI_CASCADE_" + k, raising=False)
        for k, v in SETTINGS[setting][0].items():
            monkeypatch.setenv(k, v)
        for dim, m, n, g in SETTINGS[setting][2]:
            plan = device.cascade_plan(2000, 700, dim, m, n, g)
            assert {k: plan[k] for k in wants} == wants, (setting, dim, m, n, g, plan)
