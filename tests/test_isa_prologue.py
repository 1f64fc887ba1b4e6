"""The decode kernels' prologues, checked in the compiled gfx950 code (no GPU needed; hipcc cross-compiles in ~10 s).

Round 4's review found that every decode launch spent its first microseconds on DEPENDENT scalar round trips: hipcc sinks each
kernel-argument fetch to its first use, so `gemm_rows_kernel` had three to four `s_load -> s_waitcnt lgkmcnt(0)` pairs in front of
its first weight-tile load and `paged_attention_kernel` six of them, a vector round trip and a barrier in front of its first K/V
load ("What's weak" 2).  Round 5 orders the arguments for kernarg preloading and fetches the rest in one burst behind
the first tile loads (gemm_rows_kernel.inc, gpt_kernels.hip); this test keeps it that way."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_skeleton  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def asm():
    return isa_skeleton.compile_to_asm(os.path.join(ROOT, "auralis_amd", "csrc", "gpt_kernels.hip"))


def test_build_preloads_kernel_arguments():
    from auralis_amd.build import FLAGS
    assert "-amdgpu-kernarg-preload-count=16" in FLAGS


def test_gemm_rows_requests_its_first_weight_tile_without_waiting_for_anything(asm):
    ks = isa_skeleton.kernels(asm, "gemm_rows_kernel")
    assert len(ks) >= 20, "every (shape, epilogue, arithmetic) instantiation of the decode GEMM"
    for name, body in ks:
        p = isa_skeleton.prologue(body)
        assert p["found_data_load"], name
        assert p["preload_dwords"] == 14, (name, p)   # Wt, X, bias, ln_c1, out, stats_in, M | N/16, xmt | omt
        # nothing between the entry and the first global_load_dwordx4: no kernel-argument round trip, no wait on the small
        # epilogue-input loads issued first, no barrier
        assert p["scalar_waits"] == 0 and p["vector_waits"] == 0 and p["barriers"] == 0, (name, p)
        assert p["flat_loads"] == 0, (name, "a FLAT load turns every counted wait of the kernel into vmcnt(0)")


@pytest.mark.parametrize("kvh,q_loads", [("ILb0E", 1), ("ILb1E", 2)])
def test_decode_attention_is_one_scalar_round_trip_away_from_its_first_kv_load(asm, kvh, q_loads):
    ks = isa_skeleton.kernels(asm, "paged_attention_kernel" + kvh)
    assert len(ks) == 1
    name, body = ks[0]
    p = isa_skeleton.prologue(body, skip=q_loads)   # the q row is requested first; look at what precedes the first K/V load
    assert p["found_data_load"] and p["preload_dwords"] >= 9, p
    # one trip: the row's position, write block and first block ids, fetched together (scalar loads out of row_meta)
    # (the loop header carries a second s_waitcnt for the ids requested one iteration ahead: nothing is outstanding when the first
    # iteration reaches it)
    assert p["scalar_round_trips"] <= 1 and p["vector_waits"] == 0 and p["barriers"] == 0, (name, p)
    assert p["flat_loads"] == 0
    # all 2 * UN K/V requests of an iteration leave before the first wait on any of them (round 5: hipcc had sunk one V load into
    # the branch that uses it, behind a vmcnt(0))
    seq = isa_skeleton.tokens(body)
    wide = [i for i, t in enumerate(seq) if t == "L4"]
    first_kv = wide[q_loads]
    run = 0
    for t in seq[first_kv:]:
        if t == "L4":
            run += 1
        elif t.startswith("W"):
            break
    assert run == 8, (name, run)


def test_decode_attention_is_one_copy_of_its_loop(asm):
    """Round 5: every launch pulls its code through a COLD instruction cache.  hipcc had peeled the first iteration of the token loop
    and unrolled sixteen copies of expf in the final merge: 6.7 KB.  One copy of the loop and one expf in the merge are 3.1 KB (fp32
    pool); the bound leaves room for scheduling differences, not for a second copy."""
    import re
    for kvh, cap in (("ILb0E", 3600), ("ILb1E", 4700)):
        (name, body), = isa_skeleton.kernels(asm, "paged_attention_kernel" + kvh)
        size = int(re.search(r"codeLenInByte = (\d+)", body).group(1)) if "codeLenInByte" in body else None
        if size is None:   # (the marker sits behind .end_amdhsa_kernel in some layouts: fall back to counting the loop's MFMA-free body)
            size = int(re.search(re.escape(name) + r":.*?codeLenInByte = (\d+)", asm, re.S).group(1))
        assert size <= cap, (name, size)
        assert len(re.findall(r"v_exp_f32", body)) <= 2 * 4 + 1, (name, "copies of expf: two per token step, four steps, one in the merge")


def test_no_gpt_kernel_spills_or_uses_flat_loads(asm):
    """Every kernel of the GPT translation unit keeps its state in registers (no scratch: private segment 0) and addresses global
    memory with global_ / buffer_ instructions -- one flat_load makes every later counted wait of its kernel a vmcnt(0) (round 5)."""
    import re
    ks = isa_skeleton.kernels(asm, "")
    assert len(ks) >= 60
    for name, body in ks:
        priv = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert priv and int(priv[0]) == 0, (name, "scratch bytes per lane", priv)
        assert "flat_load" not in body and "scratch_" not in body, name


def test_no_vocoder_kernel_spills():
    """twenty instantiations of the register-staged fp16 conv kernel (every 64-channel tile, conv_pre among them: on the
    hot path) carried 32 spilled VGPRs and 76 B of scratch per lane, and no test looked at the vocoder unit.  No kernel of ANY unit of
    the library may use scratch or spill -- the engine launches any of them depending on shapes and A/B switches.  Read from the
    compiler's own resource report of the in-tree build (auralis_amd/build.py keeps hipcc's -Rpass-analysis=kernel-resource-usage
    remarks next to each object), so the four-minute vocoder unit is not compiled a second time."""
    from auralis_amd.build import SOURCES, kernel_resources
    n = 0
    for unit in SOURCES:
        res = kernel_resources(unit)
        # (an SGPR spill goes to lanes of a VGPR, not to memory: reported by the compiler, not a scratch access)
        bad = {k: v for k, v in res.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0)}
        assert not bad, (unit, bad)
        n += len(res)
    assert len(kernel_resources("vocoder_kernels.hip")) >= 60 and n >= 150, n


def test_dma_conv_tiles_are_the_launched_ones_and_keep_their_occupancy():
    """The LDS-DMA conv kernel is compiled for exactly the tiles the launcher picks: the 64-channel eight-wave tile of every k >= 3
    conv (two workgroups per CU: <= 128 registers) and the four-wave tile of the transposed convs; the 128- and 32-channel tiles
    were measured and removed and do not come back as dead instantiations.  The fused ResBlock rounds fit their 512-thread
    workgroups (<= 128)."""
    import re
    from auralis_amd.build import kernel_resources
    res = kernel_resources("vocoder_kernels.hip")

    def regs(v):
        return v["vgprs"] + v.get("agprs", 0)
    # <KS, DIL, MT, NBUF, NWV, EPIH> of every instantiation
    dma = [tuple(int(g) for g in re.search(r"conv1d_dma_f16_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", k).groups())
           for k in res if "conv1d_dma_f16_kernel" in k]
    want = {(ks, dil, 64, 3 if ks == 3 else 2, 8, 1) for ks in (3, 7, 11) for dil in (1, 3, 5)} | {(2, 1, 64, 4, 4, 0)}
    assert len(dma) == 10 and set(dma) == want, sorted(set(dma) ^ want)
    narrow = {k: v for k, v in res.items() if "conv1d_dma_f16_kernelILi3ELi1ELi64ELi3ELi8E" in k}
    rounds = {k: v for k, v in res.items() if "resblock_round_f16_kernel" in k}
    assert len(narrow) == 1 and len(rounds) == 18, (len(narrow), len(rounds))
    assert all(regs(v) <= 128 for v in narrow.values()), narrow
    assert all(regs(v) <= 128 for v in rounds.values()), {k: regs(v) for k, v in rounds.items() if regs(v) > 128}
