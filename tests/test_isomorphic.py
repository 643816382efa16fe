"""isomorphic and invert without a GPU: the restatement tests/isomorphic_ref.py against the known answers of K22, the verdict
mix of the seeded parity families, props::invert against the restated invert_properties, and the plumbing — header,
bindings, counters, the C++ mirror with its example, the narrow limits stated in three places."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rustfst_amd
from rustfst_amd import _lib

from oracle.model import KDELTA
from oracle.model.props import ALL, B

import helpers
import isomorphic_cases as K
import isomorphic_ref as R

ROOT = helpers.ROOT
COUNTERS = ("levels", "narrow_launches", "wide_launches", "narrow_levels", "max_level_width", "pairs", "events", "wave_pairs",
            "big_states_sorted", "nondet_marks")
DECLARED = {
    "wfst_fst_invert": "wfst_ctx* ctx, wfst_fst* fst",
    "wfst_isomorphic": "wfst_ctx* ctx, const wfst_fst* fst1, const wfst_fst* fst2, const wfst_isomorphic_config* cfg, int* is_isomorphic",
    "wfst_ctx_get_isomorphic_counters": "wfst_ctx* ctx, " + ", ".join("uint64_t* " + k for k in COUNTERS),
}


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", K.k22_cases(), ids=lambda c: c[0])
def test_restatement_reproduces_k22(case):
    name, f1, f2, delta, expected = case
    assert R.verdict(f1, f2, KDELTA if delta is None else delta) == expected


def test_k22_covers_the_order_sensitive_cases():
    names = [c[0] for c in K.k22_cases()]
    for letter in "abcdefghij":
        assert any(n.startswith(letter + "_") for n in names), letter
    assert sum(n.startswith("py_") for n in names) == 3
    verdicts = [c[4] for c in K.k22_cases()]
    assert 1 in verdicts and 0 in verdicts and sum(isinstance(v, str) for v in verdicts) >= 3
    # (a) is the same pair of operands both ways round
    a = {c[0]: c for c in K.k22_cases()}
    assert a["a_two_to_one"][1] == a["a_one_to_two"][2] and a["a_two_to_one"][4] != a["a_one_to_two"][4]


def test_restated_invert_on_k22():
    inv = K.k22()["invert"]
    got, exp = R.invert(K.from_spec(inv["input"])), K.from_spec(inv["expected"])
    assert (got["rows"], got["finals"], got["start"]) == (exp["rows"], exp["finals"], exp["start"])
    assert R.invert(got)["rows"] == K.from_spec(inv["input"])["rows"]


def test_tr_compare_is_ordered_float():
    nan, inf = float("nan"), float("inf")
    assert R.tr_compare([1, 1, -0.0, 2], [1, 1, 0.0, 2]) == 0 and R.tr_compare([1, 1, -0.0, 3], [1, 1, 0.0, 2]) == 1
    assert R.tr_compare([1, 1, nan, 0], [1, 1, inf, 9]) == 1 and R.tr_compare([1, 1, nan, 0], [1, 1, nan, 0]) == 0
    assert R.tr_compare([1, 2, 5.0, 0], [2, 1, 0.0, 0]) == -1 and R.tr_compare([1, 2, 5.0, 0], [1, 1, 9.0, 0]) == 1
    assert not R.approx_equal(inf, inf, KDELTA) and R.approx_equal(0.0, 1.0 / 1024.0, KDELTA)


@pytest.mark.parametrize("name", sorted(K.FAMILIES))
def test_families_yield_every_verdict(name):
    """the restatement alone gives 1, 0 and the error in at least a tenth of the family's cases each: a device path that
    always answered the same could not pass tests/test_isomorphic_gpu.py"""
    cases = K.family(name)
    verdicts = [R.verdict(f1, f2) for _, f1, f2 in cases]
    count = {1: verdicts.count(1), 0: verdicts.count(0), "KO": sum(isinstance(v, str) for v in verdicts)}
    assert len(cases) >= 50 and all(10 * c >= len(cases) for c in count.values()), count
    assert all(5 <= len(f1["rows"]) <= 400 for _, f1, _ in cases)
    kinds = {n.rsplit("-", 1)[1] for n, _, _ in cases}
    assert kinds == set(K.MUTATIONS) | {"permuted"}


# ---------------------------------------------------------------- props::invert
def test_invert_props_against_the_restatement(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "invert_props_check"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rustfst_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "invert_props_check.cpp")])
    rng = np.random.default_rng(2222)
    words = [0] + [1 << b for b in range(64)] + [int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) for _ in range(200)]
    words += [ALL, ALL | 3, (1 << 64) - 1]
    out = subprocess.run([str(exe)] + ["%x" % w for w in words], capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(words) + 1
    for w, line in zip(words, out):
        got_w, got = (int(x, 16) for x in line.split())
        assert got_w == w
        assert got & ALL == R.invert_properties(w & ALL), hex(w)  # the trinary bits: the reference's rule
        assert got & ~ALL == w & ~ALL, hex(w)                      # what lies outside them is carried, as props::project does
    for name in B:  # an involution on every defined bit
        assert R.invert_properties(R.invert_properties(1 << B[name])) == 1 << B[name]
    assert R.invert_properties(R.I_LABEL_SORTED | R.NO_O_EPSILONS | R.ACCEPTOR) == R.O_LABEL_SORTED | R.NO_I_EPSILONS | R.ACCEPTOR


# ---------------------------------------------------------------- plumbing
def test_declarations_bindings_and_counters_agree():
    header = read("include", "wfst.h")
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, params in DECLARED.items():
        assert helpers.header_params(header, name) == params, name
        assert name in bound and bound[name][0] is C.c_int
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    assert bound["wfst_fst_invert"][1] == [vp, vp]
    assert bound["wfst_isomorphic"][1] == [vp, vp, vp, C.POINTER(_lib.IsomorphicConfig), C.POINTER(C.c_int)]
    assert bound["wfst_ctx_get_isomorphic_counters"][1] == [vp] + [u64p] * len(COUNTERS)
    assert _lib.ISOMORPHIC_COUNTERS == COUNTERS
    assert [f for f, _ in _lib.IsomorphicConfig._fields_] == ["delta"]
    assert re.search(r"typedef struct \{ float delta; \} wfst_isomorphic_config;", header)
    # the getter stays outside the table of the *_stats families, its struct outside the *Stats structs
    assert "wfst_ctx_get_isomorphic_counters" not in {s for s, _ in _lib.COUNTERS.values()}
    common = read("rustfst_amd", "csrc", "common.h")
    m = re.search(r"struct IsomorphicCounters \{(.*?)\} isomorphic;", common, re.S)
    assert m and re.findall(r"(\w+) = 0", m.group(1)) == list(COUNTERS)
    api = read("rustfst_amd", "csrc", "api.cpp")
    m = re.search(r"get_counters\(ctx, &wfst_ctx::isomorphic, \{([^}]*)\}\)", api)
    assert m and re.findall(r"\w+", m.group(1)) == list(COUNTERS)
    note = re.search(r"#define\s+WFST_ABI_VERSION\s+7\b(.*)", header).group(1).split("; 6:")[0]
    assert all(name in note for name in DECLARED)
    assert "isomorphic.hip" in read("rustfst_amd", "build.py")
    for name in ("invert", "isomorphic"):
        assert name in rustfst_amd.__all__ and callable(getattr(rustfst_amd, name))
        assert callable(getattr(rustfst_amd.DeviceFst, name)) and callable(getattr(rustfst_amd.VectorFst, name))
    assert callable(rustfst_amd.Context.isomorphic_stats)


def test_library_exports_the_symbols(wfst_lib):
    for name in DECLARED:
        assert hasattr(wfst_lib, name)
    assert wfst_lib.wfst_abi_version() == 7
    helpers.null_ctx_is_ko(wfst_lib, "wfst_ctx_get_isomorphic_counters", len(COUNTERS))
    res = C.c_int(7)
    assert "null" in helpers.ko_message(wfst_lib.wfst_isomorphic(None, None, None, None, C.byref(res))) and res.value == 7
    assert "null" in helpers.ko_message(wfst_lib.wfst_fst_invert(None, None))


def test_cpp_mirror_and_example_compile():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for path in (os.path.join(ROOT, "examples", "isomorphic_tests.cpp"), os.path.join(ROOT, "include", "wfst.hpp")):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"), path],
                       check=True, capture_output=True)


def test_narrow_limits_are_stated_alike():
    kernel, header, design = read("rustfst_amd", "csrc", "isomorphic.hip"), read("include", "wfst.h"), read("DESIGN.md")
    for name, value in (("ISOMORPHIC_NARROW_PAIRS", K.NARROW_PAIRS), ("ISOMORPHIC_NARROW_EVENTS", K.NARROW_EVENTS)):
        assert int(re.search(r"constexpr uint32_t %s = (\d+);" % name, kernel).group(1)) == value
        assert int(re.search(r"#define WFST_%s (\d+)" % name, header).group(1)) == value
        assert int(re.search(r"`%s` = (\d+)" % name, design).group(1)) == value
    assert int(re.search(r"constexpr uint32_t ISOMORPHIC_WAVE_ARCS = (\d+);", kernel).group(1)) == K.WAVE_ARCS
    assert int(re.search(r"constexpr uint32_t ISO_RANK_MAX = (\d+);", kernel).group(1)) == K.RANK_MAX
    assert "WFST_ISOMORPHIC_PATH" in design and "3.17" in design
