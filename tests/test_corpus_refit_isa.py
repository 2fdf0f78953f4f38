"""CPU guard on the code hipcc generates for the kernels behind Corpus.refit_idf (no GPU needed: hipcc cross-compiles gfx950).
The column count (string_grouper_amd/csrc/sg_vectorize.hip) must read the indices 16 bytes at a time and count in LDS; the
reweigh kernel must keep K2's shape -- the sum of squares down a chain of row_shr:1 DPP moves, 32 of them for the two halves of
sixteen doubles -- with the one atomic on the mismatch word; none of them, nor the gather of the norms in sg_csr_ops.hip, may
touch scratch."""
import re

import pytest

from tests.test_csr_select_isa import _asm, _kernels


@pytest.fixture(scope="module")
def vectorize_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sg_vectorize.hip")


def _no_scratch(body, meta, name):
    assert not re.search(r"\bscratch_(load|store)", body), name
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta), name


def test_the_column_count_reads_sixteen_bytes_a_lane_and_counts_in_lds(vectorize_asm):
    found = _kernels(vectorize_asm, "column_count_lds_kernel")
    assert len(found) == 1, "kernel not found"
    name, body, meta = found[0]
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) == 1            # the body's unit of four indices
    assert len(re.findall(r"\bds_add_u32\b", body)) >= 4
    assert not re.search(r"\bglobal_atomic", body) and not re.search(r"\bflat_(load|store)", body)
    _no_scratch(body, meta, name)


@pytest.mark.parametrize("value_type", ["f", "d"])
def test_the_reweigh_kernel_keeps_k2s_shape(vectorize_asm, value_type):
    found = _kernels(vectorize_asm, "reweigh_rows16_kernelI%sE" % value_type)
    assert len(found) == 1, "kernel not found"
    name, body, meta = found[0]
    assert len(re.findall(r"\bv_mov_b32_dpp\b[^\n]*row_shr:1", body)) == 32
    assert len(re.findall(r"\bglobal_atomic_add\b", body)) == 1              # the mismatch word, nothing else
    assert len(re.findall(r"\bglobal_atomic_umax\b", body)) == 2             # the two words K2 reduces
    assert re.search(r"\bv_rndne_f64", body)                                 # the count: rint in double
    _no_scratch(body, meta, name)


def test_the_gather_of_the_norms_uses_no_scratch(tmp_path_factory):
    found = _kernels(_asm(tmp_path_factory, "sg_csr_ops.hip"), "gather_row_norms_kernel")
    assert len(found) == 1, "kernel not found"
    name, body, meta = found[0]
    _no_scratch(body, meta, name)
