"""The fp16-pair split and the buffer helpers are defined once, in csrc/common.h (Precision).

A kernel file that pastes its own copy of one of them, or a prefixed twin, fails here (source scan, no compute)."""
import glob
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "debiasing-multi-modal_amd", "csrc")
FUNCTIONS = ("desc", "glds16", "scale_exp", "pow2f", "split2h_pair", "pack2", "frag")
CONSTANTS = ("OOR", "EXT_LIM")


def _sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if path.endswith((".hip", ".h", ".inc")):
            txt = open(path).read()
            out[os.path.basename(path)] = re.sub(r"//[^\n]*", "", txt)        # comments may speak of the names
    return out


SOURCES = _sources()


def _where(pattern):
    return sorted((name, len(re.findall(pattern, txt))) for name, txt in SOURCES.items() if re.search(pattern, txt))


def test_sources_found():
    assert "common.h" in SOURCES and len(SOURCES) >= 20


@pytest.mark.parametrize("name", FUNCTIONS)
def test_device_helper_defined_once_in_common_h(name):
    # a __device__ function definition of exactly this name: declarator, parameter list, opening brace
    assert _where(r"__device__\s[^;(){}]*?\b%s\s*\([^;{}]*\)\s*\{" % name) == [("common.h", 1)]


@pytest.mark.parametrize("name", CONSTANTS)
def test_constant_defined_once_in_common_h(name):
    assert _where(r"\bconstexpr\s[^;=(){}]*?\b%s\s*=" % name) == [("common.h", 1)]


@pytest.mark.parametrize("name", FUNCTIONS + CONSTANTS + ("pow2", "split_pair", "f16x8", "u32x4"))
def test_no_stem_prefixed_twin(name):
    assert _where(r"\bstem_%s\b" % name) == []


# What the persistent 256-tile kernels share (csrc/persistent_tiles.h, csrc/fp16_ring.inc): a kernel file that carries
# its own copy of the XCD split, the slice store, the slice sum or the fp16 ring's phase again fails here.
@pytest.mark.parametrize("statement,where", [
    ("const int tq = ", "common.h"),                                  # the split of tile ids over the XCDs (xcd_first)
    ("raw_buffer_store_b128(v, rsP", "persistent_tiles.h"),           # slice_store
    ("src += 32 * 512", "persistent_tiles.h"),                        # slice_sum
    ("fb1[ks] = *(const u32x4*)(base + 2 * PH_HALF + boff[ks])", "fp16_ring.inc"),   # the fp16 ring's phase
])
def test_persistent_tile_statement_stated_once(statement, where):
    assert _where(re.escape(statement)) == [(where, 1)]


@pytest.mark.parametrize("name", ("tile_walk", "work_item", "work_slices", "slice_store", "slice_sum", "absmax_fold", "ring_rows"))
def test_persistent_tile_helper_defined_once(name):
    assert _where(r"__device__\s[^;(){}]*?\b%s\s*\([^;{}]*\)\s*\{" % name) == [("persistent_tiles.h", 1)]


# What the k-means sums and the label sums share (csrc/label_sums.h; DESIGN.md, sections 6c and 6e): the partition, the unit body, the
# fixed-order merge.  The promise is the same bits on every call; a second copy of the order could move without the other.
def test_wave_sum_f64_defined_once_in_common_h():
    assert _where(r"__device__\s[^;(){}]*?\bwave_sum_f64\s*\([^;{}]*\)\s*\{") == [("common.h", 1)]


@pytest.mark.parametrize("name", ("wave_unit", "unit_sums", "quarter_sums", "merge_sum", "merge_count"))
def test_label_sums_helper_defined_once(name):
    assert _where(r"__device__\s[^;(){}]*?\b%s\s*\([^;{}]*\)\s*\{" % name) == [("label_sums.h", 1)]


@pytest.mark.parametrize("statement", [
    "((quarter[0][lane] + quarter[1][lane]) + quarter[2][lane]) + quarter[3][lane]",   # the merge order (merge_sum)
    "acc[j][e] = fma(w, v[e], acc[j][e])",                                            # the predicated add (unit_sums)
    "long long p = (UNITS + sl - 1) / sl",                                            # the partition (ranges)
])
def test_label_sums_statement_stated_once(statement):
    assert _where(re.escape(statement)) == [("label_sums.h", 1)]


# What the pairwise-kernel family shares in the library (csrc/pairdist.hip, csrc/pairdist_ring.inc): the ring's
# source map, the accumulators' d^2 step, the operand check and the prepare step of every pass.  A further entry or tile kernel that
# restates one of them fails here.
@pytest.mark.parametrize("statement,where", [
    ("const int kt = isA ? (t < p.T ? t : t - p.T)", "pairdist_ring.inc"),       # ring_src: the three products' K tiles inside a row of P
    ("fmaf(-2.f, acc[i][0][r], rn + cn0)", "pairdist.hip"),                      # PAIRDIST_ACC_TO_D2
    ("hipLaunchKernelGGL(pairdist_absmax_kernel", "pairdist.hip"),               # prepare
])
def test_pairdist_statement_stated_once(statement, where):
    assert _where(re.escape(statement)) == [(where, 1)]


def test_pairdist_row_limit_stated_once():
    # check_operands; the other analysis kernels state their own limit (common.h: dbmm_rows_shape)
    assert SOURCES["pairdist.hip"].count("N > (1 << 23)") == 1
