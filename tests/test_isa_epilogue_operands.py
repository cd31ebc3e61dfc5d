"""Static check (no GPU; assembly built as tests/test_isa_static.py builds it) that the data-gradient GEMMs request their epilogue's
global operands -- ReLU mask, `+=` base, O / O32 of the row-dot -- all together in the LAST step of the K loop and that the epilogue's store
loop holds no load any more.  Left to itself (or after an innocent edit) the compiler sinks such loads to their use, and the tail of every
block becomes a chain of 4 - 8 serialised round trips again (NOTEBOOK.md B).

A 16-byte operand piece is a plain global_load_dwordx4; the operand stages of these kernels are global_load_lds_dwordx4 (another mnemonic),
the pooled-gradient epilogue loads 8-byte selection codes, and the element-wise fallback epilogue of the four-wave kernel loads 2 and 8
bytes.  The K loops of these kernels write LDS by DMA only, so the first ds_write of a kernel is the staging of its accumulators: "every
plain 16-byte load in front of the first ds_write" is exactly "requested before the block is staged, nothing loaded in the store loops".
The request also stays BEHIND the ring's stages: in front of them the first counted wait waits for these cold lines (vmcnt retires in
order), which was measured to move the latency from the tail to the head of the block (profiles/nn_epilogue_operands_ab.txt).

Registers.  The eight-wave kernels are built for two workgroups per CU (__launch_bounds__(512, 2)): 16 waves, four per SIMD, 512 / 4 = 128
registers.  The four-wave ring kernel takes 3 x 16 KB of LDS per workgroup, so three workgroups share a CU's 160 KB whatever the registers
(the parent's 60 would allow eight): three waves per SIMD, 512 / 3 rounded down to the allocation granule of 8 = 168 registers keep them."""
import re

import pytest

from test_isa_static import _asm, _kernel, _ops


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    tmp, done = str(tmp_path_factory.mktemp("isa_epi")), {}

    def get(name):
        if name not in done:
            done[name] = _asm(tmp, name)
        return done[name]
    return get


@pytest.mark.parametrize("source,kernel,loads,max_vgpr", [
    # two operand registers sets (mask or O or O32 low | `+=` base or O32 high) x four pieces per thread of the 128 x 128 block
    ("gemm_big.hip", r"gemm_big_nn_kernelILi2E", 8, 128),
    ("gemm_big.hip", r"gemm_big_nn_kernelILi4E", 8, 128),
    # ... x two pieces per thread of the 64 x 64 tile
    ("gemm_nn.hip", r"gemm_nn_kernelIttLi64ELi3E", 4, 168),
])
def test_epilogue_operands_are_requested_in_the_last_k_step(asm, source, kernel, loads, max_vgpr):
    seg = _kernel(asm(source), kernel)
    ops = _ops(seg)
    plain = [i for i, (o, _) in enumerate(ops) if o == "global_load_dwordx4"]
    assert len(plain) == loads, [ops[i][1] for i in plain]
    staged = [i for i, (o, _) in enumerate(ops) if o.startswith("ds_write")]
    dma = [i for i, (o, _) in enumerate(ops) if o == "global_load_lds_dwordx4"]
    assert staged and dma
    assert max(plain) < staged[0], "an epilogue operand is loaded behind the staging of the block (inside the store loop again?)"
    assert min(plain) > dma[0], "the epilogue operands are requested in front of the ring: its first counted wait would wait for them"
    # ... and the compiler waits for them where they are used, not in the K loop: no vmcnt wait between the request and the staging
    assert not [t for o, t in ops[min(plain):staged[0]] if o == "s_waitcnt" and "vmcnt" in t]
    meta = "\n".join(seg)
    nv = re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta)
    sc = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta)
    assert sc and int(sc.group(1)) == 0, sc and sc.group(1)
    assert nv and int(nv.group(1)) <= max_vgpr, nv and nv.group(1)
