"""CPU guard on the code hipcc generates for the kernels behind a kept self-join (no GPU needed: hipcc cross-compiles gfx950).
The row copies of sg_topn_concat_rows / sg_topn_put_rows (string_grouper_amd/csrc/sg_corpus.hip) move 16 bytes a lane where the
strides allow it; sg_topn_forget reads its dead list from LDS when it fits, as sg_topn_drop_columns does with the filter the two
share; sg_csr_take_rows' descriptor kernel (sg_csr_ops.hip) and all the others touch no scratch and make no generic-address
access."""
import re

import pytest

from tests.test_csr_select_isa import _asm, _kernels


@pytest.fixture(scope="module")
def corpus_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sg_corpus.hip")


@pytest.fixture(scope="module")
def csr_ops_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sg_csr_ops.hip")


def _clean(found):
    for name, body, meta in found:
        assert not re.search(r"\bscratch_(load|store)", body), name
        assert not re.search(r"\bflat_(load|store)", body), name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta), name


@pytest.mark.parametrize("value_type,wide", [("f", 2), ("d", 3)])
def test_the_row_copy_moves_sixteen_bytes_a_lane_where_the_strides_allow(corpus_asm, value_type, wide):
    vec = _kernels(corpus_asm, "topn_copy_rows_kernelI%sLb1EE" % value_type)
    plain = _kernels(corpus_asm, "topn_copy_rows_kernelI%sLb0EE" % value_type)
    assert len(vec) == 1 and len(plain) == 1, "kernel not found"
    _clean(vec + plain)
    # columns + values of four entries: 2 (f32) / 3 (f64) 16-byte loads and as many stores
    assert len(re.findall(r"\bglobal_load_dwordx4\b", vec[0][1])) >= wide
    assert len(re.findall(r"\bglobal_store_dwordx4\b", vec[0][1])) >= wide


def test_the_forget_kernels_keep_a_short_dead_list_in_lds_and_use_no_scratch(corpus_asm):
    found = _kernels(corpus_asm, "forget_kernel")
    assert len(found) == 4, [name for name, _, _ in found]          # f32 / f64 x dead list in LDS / in memory
    _clean(found)
    for name, body, _ in found:
        in_lds = "Lb1EE" in name
        assert bool(re.search(r"\bds_read", body)) == in_lds, name   # both searches (the row's place, the filter) in LDS, or none
    _clean(_kernels(corpus_asm, "short_rows_kernel"))


def test_the_filter_shared_with_drop_columns_still_reads_its_list_from_lds(corpus_asm):
    found = _kernels(corpus_asm, "drop_columns_kernel")
    assert len(found) == 4
    _clean(found)
    for name, body, _ in found:
        assert bool(re.search(r"\bds_read", body)) == ("Lb1EE" in name), name


def test_the_descriptor_kernel_of_take_rows_uses_no_scratch(csr_ops_asm):
    found = _kernels(csr_ops_asm, "csr_take_parts_kernel")
    assert len(found) == 1, "kernel not found"
    for name, body, meta in found:
        assert not re.search(r"\bscratch_(load|store)", body), name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta), name
