"""No GPU: the in-place update entries of include/emdr2_mips.h validate their arguments before any launch, the block-norm table has one
float per 256-row block of the padded image, and the parser knows --index-refresh-in-place."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def test_block_norm_bytes(lib):
    n = ctypes.c_size_t()
    assert lib.emdr2_mips_block_norm_bytes(21015324, ctypes.byref(n)) == 0
    assert n.value == ((21015324 + 511) // 512 * 512) // 256 * 4
    assert lib.emdr2_mips_block_norm_bytes(1, ctypes.byref(n)) == 0 and n.value == 8
    assert lib.emdr2_mips_block_norm_bytes(10, None) == -1
    assert lib.emdr2_mips_block_norm_bytes(-1, ctypes.byref(n)) == -1


def test_update_entries_reject_bad_arguments_before_any_launch(lib):
    p = ctypes.c_void_p(4096)                                           # never dereferenced: every call below fails its validation
    # null pointers
    assert lib.emdr2_mips_block_norms(None, 1000, 768, 0, 4, p, None) == -1
    assert lib.emdr2_mips_block_norms(p, 1000, 768, 0, 4, None, None) == -1
    assert lib.emdr2_mips_update_rows(None, 10, 768, 0, 1000, p, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 768, 0, 1000, None, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 768, 0, 1000, p, None, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 768, 0, 1000, p, p, None, None, None, None, None) == -1
    # a shadow image without its table / its flag
    assert lib.emdr2_mips_update_rows(p, 10, 768, 0, 1000, p, p, p, p, None, p, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 768, 0, 1000, p, p, p, p, p, None, None) == -1
    # ranges past the shard / the table
    assert lib.emdr2_mips_update_rows(p, 10, 768, 991, 1000, p, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 768, -1, 1000, p, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, -1, 768, 0, 1000, p, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_block_norms(p, 1000, 768, 0, 5, p, None) == -1          # 1000 rows pad to 1024: 4 blocks
    assert lib.emdr2_mips_block_norms(p, 1000, 768, -1, 2, p, None) == -1
    # bad dim; the seal's dim % 256 == 0 applies only with a shadow
    assert lib.emdr2_mips_block_norms(p, 1000, 100, 0, 4, p, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 100, 0, 1000, p, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 32, 0, 1000, p, p, p, None, None, None, None) == -1
    assert lib.emdr2_mips_update_rows(p, 10, 96, 0, 1000, p, p, p, ctypes.c_void_p(8192), ctypes.c_void_p(8192), p, None) == -1
    # nothing to do is not an error (and launches nothing)
    assert lib.emdr2_mips_update_rows(p, 0, 768, 1000, 1000, p, p, p, None, None, None, None) == 0
    assert lib.emdr2_mips_block_norms(p, 1000, 768, 4, 0, p, None) == 0


def test_parser_knows_the_in_place_refresh_flag():
    from emdr2_amd import arguments
    base = ("--task OPENQA --num-layers 2 --hidden-size 128 --num-attention-heads 2 --max-position-embeddings 64 --seq-length 64 "
            "--decoder-seq-length 32 --batch-size 4 --lr 2e-4 --async-indexer").split()
    assert arguments.parse_args(base).index_refresh_in_place is False            # the atomic swap stays the default
    assert arguments.parse_args(base + ["--index-refresh-in-place"]).index_refresh_in_place is True
    with pytest.raises(SystemExit):
        arguments.parse_args(base + ["--index-refresh-in-place", "--index-refresh-somewhere-else"])
    help_text = " ".join(arguments.get_parser().format_help().split())
    assert "--index-refresh-in-place" in help_text and "MIX of two embedding generations" in help_text
