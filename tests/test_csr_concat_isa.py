"""CPU guard on the code hipcc generates for sg_csr_concat's kernel (string_grouper_amd/csrc/sg_csr_ops.hip; no GPU needed:
hipcc cross-compiles gfx950): the copy of indices and values is a pass over the corpus's bytes, so it must stay 16 bytes
wide on both sides -- global (not flat) loads at the source's own alignment, aligned stores -- and touch no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "string_grouper_amd", "csrc", "sg_csr_ops.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "csr_ops.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
           "-S", "--cuda-device-only", "-o", str(out), SRC]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


@pytest.mark.parametrize("value_type,wide", [("f", 2), ("d", 3)])
def test_the_concat_kernel_copies_sixteen_bytes_at_a_time_without_scratch(asm, value_type, wide):
    m = re.search(r"^(_ZN\w*csr_concat_kernelI%sEE\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % value_type, asm, re.M | re.S)
    assert m, "kernel not found"
    name, body = m.group(1), m.group(2)
    # indices + values of a unit of four entries: 2 (f32) / 3 (f64) 16-byte loads from the parts, as many aligned stores
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) >= wide
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= wide
    assert not re.search(r"\bflat_(load|store)", body), "a generic-address access: the parts' pointers lost their address space"
    assert not re.search(r"\bscratch_(load|store)", body)
    meta = asm[asm.index(".amdhsa_kernel " + name):]
    meta = meta[:meta.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", meta)
