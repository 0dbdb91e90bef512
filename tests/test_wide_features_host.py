"""Host side of the column-sliced pooling and the fused final pass at feature widths other than 512 (no GPU needed): which kernel
family each width resolves to, which widths the fused gather + classify takes, the flags size of the chained launch, the binding."""
import ctypes

import pytest

from geopurify_amd import _lib


def test_resolver_sends_256_and_768_to_the_matrix_cores():
    from geopurify_amd import pipeline as pl
    S = dict(K=96, num_iters=19, tile_rows=8, block_rows=64)
    table = [
        ("auto", 768, "cs"), ("auto", 256, "cs"),
        ("auto", 1024, "tiles"),                                        # unchanged: the cs kernels run there by name only
        ("auto", 512, "cs"),
        ("mfma_cs", 768, "cs"), ("mfma_cs", 256, "cs"), ("mfma_cs", 1024, "cs"),
        ("mfma_chain", 768, "chain"), ("mfma_chain", 256, "chain"), ("mfma_chain", 1024, "chain"),
        ("ell", 768, "ell"), ("tiles", 768, "ell"),
    ]
    for mode, D, family in table:
        assert pl.resolve_pool_mode(mode, D=D, **S) == family, (mode, D)
    assert pl.resolve_pool_mode("auto", D=768, **dict(S, num_iters=2)) == "ell"   # as at 512: the matrix cores from 3 applications on
    assert pl.resolve_pool_mode("auto", D=768, **dict(S, K=128)) == "ell"         # K > 96: not the cs kernels
    assert pl.resolve_pool_mode("auto", D=1024, **dict(S, num_iters=1)) == "ell"
    for D in (640, 128, 1280, 64):
        with pytest.raises(ValueError, match="K <= 96"):
            pl.resolve_pool_mode("mfma_cs", D=D, **S)
        with pytest.raises(ValueError, match="K <= 96"):
            pl.resolve_pool_mode("mfma_chain", D=D, **S)
    with pytest.raises(ValueError):
        pl.resolve_pool_mode("mfma_cs", D=768, **dict(S, K=128))


def test_fused_classify_widths():
    from geopurify_amd import ops
    assert ops.can_gather_rows_classify(768, 19) and not ops.can_gather_rows_classify(768, 32)
    assert ops.can_gather_rows_classify(1024, 16) and not ops.can_gather_rows_classify(1024, 17)
    assert ops.can_gather_rows_classify(512, 19) and not ops.can_gather_rows_classify(1088, 1) and not ops.can_gather_rows_classify(800, 1)
    assert [d for d in (128, 256, 512, 640, 768, 896, 1024, 1280) if ops.pool_cs_width_ok(d)] == [256, 512, 768, 1024]


def test_chain_flag_words_per_width():
    lib = _lib.load()
    lib.gp_pool_cs_chain_flag_words_d.restype = ctypes.c_size_t
    nv, rpb = 1000, 128                                                 # 8 row blocks
    for d, slices in ((256, 1), (512, 2), (768, 3), (1024, 4)):
        assert lib.gp_pool_cs_chain_flag_words_d(nv, rpb, d) == 32 + slices * 8
    assert lib.gp_pool_cs_chain_flag_words_d(nv, rpb, 512) == lib.gp_pool_cs_chain_flag_words(nv, rpb)
    for d in (0, 128, 640, 1280):
        assert lib.gp_pool_cs_chain_flag_words_d(nv, rpb, d) == 0
    assert lib.gp_pool_cs_chain_flag_words_d(nv, 8, 768) == 0          # rows per block outside 16..128


def test_new_symbol_is_declared_exported_and_bound():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "geopurify_hip.h")).read(), flags=re.S)
    assert re.search(r"\bgp_pool_cs_chain_flag_words_d\s*\(", txt)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gp_pool_cs_chain_flag_words_d")
    assert "gp_pool_cs_chain_flag_words_d" in _lib.SIGNATURES
