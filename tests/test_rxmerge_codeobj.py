"""vp_rx_merge's kernels (vp_rxmerge.hip) as they ship in the gfx950 code
object of vigor_amd/libvigpath.so, from the kernels' metadata alone (the code
objects found as test_codeobj finds them): both are there, neither keeps a
private segment or a dynamic stack, and their LDS is the queues' staged
records -- at most 1 KiB, so it never limits how many blocks a CU holds.
CPU only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_codeobj import LIB, LLVM, _code_objects

KERNELS = ["rxm_rank", "rxm_scatter"]
FIELDS = ("private_segment_fixed_size", "group_segment_fixed_size", "uses_dynamic_stack")


@pytest.fixture(scope="module")
def meta():
    """{mangled name: {field: text}} of every rxm_ kernel"""
    assert os.path.exists(LIB), "libvigpath.so not built"
    assert shutil.which("llvm-readelf", path=LLVM), "ROCm LLVM tools absent"
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in _code_objects(tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co],
                                   check=True, capture_output=True, text=True).stdout
            # one metadata map per kernel: its fields stand together, .name among them
            for block in re.split(r"\n\s+- \.", notes):
                name = re.search(r"\.name:\s+(\S+)", block)
                if not name or "rxm_" not in name.group(1):
                    continue
                found[name.group(1)] = {f: m.group(1) for f in FIELDS
                                        for m in [re.search(r"\.%s:\s+(\S+)" % f, block)] if m}
    return found


def _one(meta, short):
    hits = {k: v for k, v in meta.items() if re.search(r"\d%s[EI]" % short, k)}
    assert len(hits) == 1, (short, sorted(meta))
    return next(iter(hits.values()))


@pytest.mark.parametrize("kernel", KERNELS)
def test_rxm_kernels_keep_nothing_per_lane_in_memory(meta, kernel):
    k = _one(meta, kernel)
    assert int(k["private_segment_fixed_size"]) == 0, k
    assert k.get("uses_dynamic_stack", "false") == "false", k


@pytest.mark.parametrize("kernel", KERNELS)
def test_rxm_kernels_stage_the_queues_in_a_little_lds(meta, kernel):
    lds = int(_one(meta, kernel)["group_segment_fixed_size"])
    # 8 records of 11 64-bit words, and the rank's two windows per queue
    assert 8 * 88 <= lds <= 1024, lds


def test_every_rxm_kernel_is_covered(meta):
    assert meta and all(any(re.search(r"\d%s[EI]" % k, n) for k in KERNELS) for n in meta), \
        sorted(meta)
