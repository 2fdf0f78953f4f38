"""CPU guard on the code hipcc generates for the kernels behind Corpus.remove (no GPU needed: hipcc cross-compiles gfx950).
sg_csr_select_rows (string_grouper_amd/csrc/sg_csr_ops.hip) copies the kept rows gap by gap, which is sg_csr_concat's copy
again: it must stay 16 bytes wide on both sides -- global (not flat) loads at the source's own alignment, aligned stores --
however the dropped rows lie, and touch no scratch.  sg_topn_drop_columns (sg_corpus.hip) keeps its state in registers and
LDS: no private segment."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "string_grouper_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _asm(tmp_path_factory, source):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / (source + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
           "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, source)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


@pytest.fixture(scope="module")
def csr_ops_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sg_csr_ops.hip")


@pytest.fixture(scope="module")
def corpus_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sg_corpus.hip")


def _kernels(asm, pattern):
    """(mangled name, body, kernel descriptor) of every kernel whose mangled name matches."""
    found = []
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % pattern, asm, re.M | re.S):
        name = m.group(1)
        meta = asm[asm.index(".amdhsa_kernel " + name):]
        found.append((name, m.group(2), meta[:meta.index(".end_amdhsa_kernel")]))
    return found


@pytest.mark.parametrize("value_type,wide", [("f", 2), ("d", 3)])
def test_the_select_kernel_copies_sixteen_bytes_at_a_time_without_scratch(csr_ops_asm, value_type, wide):
    found = _kernels(csr_ops_asm, "csr_select_kernelI%sEE" % value_type)
    assert len(found) == 1, "kernel not found"
    _, body, meta = found[0]
    # indices + values of a unit of four entries: 2 (f32) / 3 (f64) 16-byte loads from the source, as many aligned stores
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) >= wide
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= wide
    assert not re.search(r"\bflat_(load|store)", body), "a generic-address access: the gaps' pointers lost their address space"
    assert not re.search(r"\bscratch_(load|store)", body)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta)


def test_the_gap_scan_of_select_rows_uses_no_scratch(csr_ops_asm):
    found = _kernels(csr_ops_asm, "csr_select_gaps_kernel")
    assert len(found) == 1, "kernel not found"
    _, body, meta = found[0]
    assert not re.search(r"\bscratch_(load|store)", body)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta)


def test_the_drop_columns_kernels_have_no_private_segment(corpus_asm):
    found = _kernels(corpus_asm, "drop_columns_kernel")
    assert len(found) == 4, [name for name, _, _ in found]          # f32 / f64 x dead list in LDS / in memory
    for name, body, meta in found:
        assert not re.search(r"\bscratch_(load|store)", body), name
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta), name
