"""CPU-only: the two lists of sdumc_amd/csrc/common.h that every kernel source registers in.

* SDUMC_PRELOAD_SOURCES against the Makefile's SRCS: every source has exactly one entry and exactly one hook line, every entry names
  a source (a source without a hook pays its deferred code-object load at its first launch, inside an epoch).
* SDUMC_PROF_VARIANTS through sdumc_profile_report: the names and their order are what bench.py and tests/gemm_cases.py read."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdumc_amd", "csrc")

# the report's names, in its order (copied from the name table the list replaced)
VARIANT_NAMES = [
    "gemm_nt_128x128", "gemm_nt_64x64", "gemm_nn_128x128", "gemm_nn_64x64", "gemm_tn_128x128", "gemm_tn_64x64",
    "gemm_small_nt", "gemm_small_nn", "gemm_small_tn",
    "gemm_bf16_nt_128x128", "gemm_bf16_nt_64x64", "gemm_bf16_nn_128x128", "gemm_bf16_nn_64x64", "gemm_bf16_tn_128x128", "gemm_bf16_tn_64x64",
    "gemm_wide_nt", "gemm_wide_tn",
    "gemm_bf16s_nt", "gemm_bf16s_tn",
    "gemm_group_tn", "gemm_group_tn_bf16",
    "gemm_rows256", "gemm_rows256_bf16",
    "gemm_wide_nt_bf16x3", "gemm_group_tn_bf16x3", "gemm_rows256_bf16x3",
    "gemm_p3_nt_bf16x3", "gemm_p3_nt_masked_bf16x3",
    "gemm_b1_nt_bf16",
]


def _macro_entries(text, macro):
    """the X(...) arguments of `#define macro(X) ...` (continuation lines joined)"""
    m = re.search(r"^#define " + macro + r"\(X\)((?:.*\\\n)*.*)$", text, re.M)
    assert m, macro
    return re.findall(r"\bX\((\w+)\)", m.group(1))


def test_every_source_is_in_the_preload_list_once():
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    stems = [s[:-len(".hip")] for s in srcs]
    assert len(stems) == len(set(stems)) and all(s.endswith(".hip") for s in srcs)
    listed = _macro_entries(open(os.path.join(CSRC, "common.h")).read(), "SDUMC_PRELOAD_SOURCES")
    assert sorted(listed) == sorted(stems), (sorted(set(stems) - set(listed)), sorted(set(listed) - set(stems)))
    for stem in stems:      # ... and each source defines its own hook, once
        hooks = re.findall(r"^SDUMC_PRELOAD_HOOK(?:_OF)?\((\w+)\)", open(os.path.join(CSRC, stem + ".hip")).read(), re.M)
        assert hooks == [stem], (stem, hooks)


def test_profile_report_names_in_a_fresh_process():
    from sdumc_amd import _lib
    code = ("import ctypes as C\n"
            "class E(C.Structure):\n"
            "    _fields_ = [('name', C.c_char_p), ('launches', C.c_int64), ('total_ms', C.c_double), ('total_flops', C.c_double)]\n"
            f"lib = C.CDLL({_lib.LIB_PATH!r})\n"
            "arr = (E * 32)()\n"
            "n = lib.sdumc_profile_report(arr, 32)\n"
            "print(n)\n"
            "for i in range(n): print(arr[i].name.decode(), arr[i].launches, arr[i].total_ms, arr[i].total_flops)\n")
    out = subprocess.check_output([sys.executable, "-c", code]).decode().split("\n")
    assert int(out[0]) == 29 == len(VARIANT_NAMES)
    rows = [l.split() for l in out[1:] if l]
    assert [r[0] for r in rows] == VARIANT_NAMES
    assert all(int(r[1]) == 0 and float(r[2]) == 0.0 and float(r[3]) == 0.0 for r in rows)
