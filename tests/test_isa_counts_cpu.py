"""tools/isa_counts.py on a hand-written piece of assembly: instruction classes, the chunk loop / tile loop / outside
regions from the branch structure (a peeled pass included), and the waits between the stores of the tile region."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASM = """
\t.globl\t_Z1kv
_Z1kv:                                  ; @_Z1kv
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v0, 0
.LBB0_1:                                ; tile loop
\ts_mul_hi_u32 s2, s3, s4
\tv_add_u32_e32 v1, v0, v0
.LBB0_2:                                ; chunk loop
\tds_read_b128 v[4:7], v1
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], v[8:11]
\tglobal_load_lds_dwordx4 v1, s[0:1]
\ts_add_u32 s0, s0, 0x3000
\ts_cbranch_scc1 .LBB0_2
; %bb.3:                                ; peeled last pass
\tv_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], v[8:11]
\ts_barrier
.LBB0_4:                                ; epilogue
\tglobal_load_dwordx4 v[12:15], v[2:3], off
\ts_waitcnt vmcnt(0)
\tv_pk_add_f32 v[8:9], v[8:9], v[12:13]
\tglobal_store_dwordx4 v[2:3], v[8:11], off
\ts_waitcnt vmcnt(0)
\tglobal_store_dwordx4 v[2:3], v[8:11], off offset:16
\ts_cbranch_scc0 .LBB0_1
; %bb.5:
\ts_endpgm
.Lfunc_end0:
"""


def load_tool():
    spec = importlib.util.spec_from_file_location("isa_counts", os.path.join(ROOT, "tools", "isa_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classes_regions_and_store_chain():
    t = load_tool()
    kernels = t.parse(ASM)
    assert list(kernels) == ["_Z1kv"]
    blocks, _ = kernels["_Z1kv"]
    assert [b.label for b in blocks] == ["entry", ".LBB0_1", ".LBB0_2", ".LBB0_4"]
    chunk, tile = t.regions(blocks)
    assert chunk == {2} and tile == {1, 3}
    n = t.total(blocks, chunk)
    # the peeled pass has no label of its own: it is laid out in the loop's block
    assert (n["mfma"], n["lds"], n["vmem"], n["salu"], n["wait"], n["valu"]) == (2, 1, 1, 2, 2, 0)
    n = t.total(blocks, tile)
    # (the fall-through exit has no label either: s_endpgm counts with the epilogue block)
    assert (n["mfma"], n["valu"], n["salu"], n["vmem"], n["wait"]) == (0, 2, 3, 3, 2)
    n = t.total(blocks, set(range(len(blocks))) - chunk - tile)
    assert (n["valu"], n["salu"]) == (1, 1)
    stores, waits, chain = t.store_chain(blocks, tile)
    assert stores == 2 and waits == 1
    assert [c.split(":")[1].split()[0] for c in chain] == ["global_load_dwordx4", "s_waitcnt", "global_store_dwordx4",
                                                           "s_waitcnt", "global_store_dwordx4"]


def test_peeled_pass_in_a_block_of_its_own_joins_the_chunk_region():
    t = load_tool()
    asm = ASM.replace("; %bb.3:                                ; peeled last pass", ".LBB0_3:")
    blocks, _ = t.parse(asm)["_Z1kv"]
    chunk, tile = t.regions(blocks)
    assert [b.label for b in blocks][3] == ".LBB0_3" and chunk == {2, 3} and tile == {1, 4}
