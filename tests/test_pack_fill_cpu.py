"""The host side of weight packing (csrc/conv_pack.hip) without a GPU: ffa_pack_desc_fill only writes a host descriptor,
ffa_pack_conv_weight_bytes only computes."""
import ctypes as C

import pytest

from flairhip import lib as L

RING, THIN, STEM = L.BCO_RING, L.BCO_THIN, L.BCO_STEM
THIN32 = 0x4000


def fill(lib, O, I, col0, ncols, k, transpose, rows, pitch, bco, dtype=L.BF16):
    desc = C.create_string_buffer(lib.ffa_pack_desc_bytes())
    fake = 0x1000  # never dereferenced on the host
    return lib.ffa_pack_desc_fill(C.addressof(desc), fake, None, fake, O, I, col0, ncols, k, k, transpose, rows, pitch, bco,
                                  lib.ffa_conv_row_group(k), dtype)


def test_operand_bytes_of_every_layout(lib):
    assert lib.ffa_pack_conv_weight_bytes(L.BF16, 128, 64, 3, 3, 64) == 128 * 64 * 9 * 2
    assert lib.ffa_pack_conv_weight_bytes(L.F32, 64, 16, 7, 7, 64) == 64 * 16 * 49 * 4
    assert lib.ffa_pack_conv_weight_bytes(L.BF16, 128, 64, 3, 3, 64 | RING) == 128 * 64 * 9 * 2
    # thin: [tiles of 16 rows][k-steps: 9 taps at 32 channels, 5 tap pairs at 16][64 lanes][16 B]
    assert lib.ffa_pack_conv_weight_bytes(L.BF16, 16, 16, 3, 3, 16 | THIN) == 1 * 5 * 1024
    assert lib.ffa_pack_conv_weight_bytes(L.BF16, 32, 32, 3, 3, 32 | THIN | THIN32) == 2 * 9 * 1024
    # stem: [14 k-steps][64 rows][64 B]
    assert lib.ffa_pack_conv_weight_bytes(L.BF16, 64, 16, 7, 7, 64 | STEM) == 14 * 64 * 64


def test_one_fill_takes_every_layout(lib):
    assert fill(lib, 70, 40, 0, 40, 3, 0, 128, 48, 64) == 0
    assert fill(lib, 70, 40, 0, 40, 3, 1, 64, 80, 64) == 0
    assert fill(lib, 70, 72, 0, 72, 3, 1, 128, 96, 64 | RING) == 0
    assert fill(lib, 19, 20, 0, 20, 3, 0, 32, 32, 32 | THIN | THIN32) == 0
    assert fill(lib, 64, 5, 0, 5, 7, 0, 64, 16, 64 | STEM) == 0


@pytest.mark.parametrize("args, text", [
    ((64, 48, 16, 24, 1, 0, 64, 32, 64), None),                                              # a column block: conv_igemm only
    ((64, 48, 40, 24, 1, 0, 64, 32, 64), "column block outside the tensor"),
    ((64, 64, 32, 32, 3, 0, 64, 32, 64 | RING), "a column block needs the conv_igemm layout"),
    ((16, 32, 0, 16, 3, 0, 16, 16, 16 | THIN), "a column block needs the conv_igemm layout"),
    ((64, 8, 0, 5, 7, 0, 64, 16, 64 | STEM), "a column block needs the conv_igemm layout"),
    ((70, 40, 0, 40, 3, 0, 64, 48, 64), "padded dims smaller than the tensor"),
    ((70, 40, 0, 40, 3, 0, 128, 48, 48), "not a multiple of block"),
    ((64, 60, 0, 60, 3, 0, 64, 80, 64 | RING), "not whole groups"),
    ((16, 16, 0, 16, 3, 0, 48, 16, 16 | THIN), "thin pack: rows 48 / pitch 16"),
    ((64, 12, 0, 12, 7, 0, 64, 16, 64 | STEM), "1..64 output and 1..8 input channels"),
    ((64, 5, 0, 5, 7, 1, 16, 64, 64 | STEM), "the stem layout is for the bf16 7x7 forward operand"),
    ((64, 64, 0, 64, 1, 0, 64, 64, 64 | RING), "the ring layout is for 3x3 kernels"),
])
def test_fill_checks(lib, args, text):
    rc = fill(lib, *args)
    if text is None:
        assert rc == 0
    else:
        assert rc != 0 and text in lib.ffa_last_error().decode()


def test_thin_layout_is_bf16_only(lib):
    assert fill(lib, 16, 16, 0, 16, 3, 0, 16, 16, 16 | THIN, dtype=L.F32) != 0
    assert "the thin layout is for bf16 3x3 kernels" in lib.ffa_last_error().decode()
