"""AffinityPredictor on a SparseTensor, the parts that need no GPU: the batched order / kernel-map entry points are declared, exported
and bound, their workspace query answers on the host, and the module rejects what it cannot run with a ValueError."""
import ctypes
import os
import re
import sys

import pytest
import torch

from geopurify_amd import _lib
from geopurify_amd.affinity_module import AffinityPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gp_coords_order_batched_workspace_bytes", "gp_coords_order_batched", "gp_kernel_map_sorted")


def _compat_me():
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import MinkowskiEngine as ME
    finally:
        sys.path.pop(0)
    return ME


def test_batched_map_symbols_declared_exported_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geopurify_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_batched_order_workspace_query_without_gpu():
    lib = _lib.load()
    small, big = lib.gp_coords_order_batched_workspace_bytes(1000), lib.gp_coords_order_batched_workspace_bytes(125_000)
    assert small >= 1000 * (8 + 4)                      # unsorted keys and row ids at least
    assert big >= 125_000 * (8 + 4) and big > small
    assert lib.gp_coords_order_batched_workspace_bytes(0) == 0


def _student(cin=38, hidden=128):
    return AffinityPredictor(input_dim=cin, embed_dim=128, hidden_dim=hidden)


@pytest.mark.parametrize("shape", [(5, 3), (5, 5), (5,)])
def test_coordinates_not_n_by_4_raise(shape):
    ME = _compat_me()
    m = _student()
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        m(ME.SparseTensor(features=torch.zeros(5, 38), coordinates=torch.zeros(shape, dtype=torch.int32)))


def test_feature_width_not_input_dim_raises():
    ME = _compat_me()
    m = _student()
    C = ME.utils.batched_coordinates([torch.arange(15).view(5, 3)])
    with pytest.raises(ValueError, match="input_dim=38"):
        m(ME.SparseTensor(features=torch.zeros(5, 39), coordinates=C))


def test_cpu_tensors_raise():
    ME = _compat_me()
    m = _student()
    C = ME.utils.batched_coordinates([torch.arange(15).view(5, 3)])
    with pytest.raises(ValueError, match="CUDA"):
        m(ME.SparseTensor(features=torch.zeros(5, 38), coordinates=C))
    with pytest.raises(ValueError, match="CUDA"):
        m.train()(ME.SparseTensor(features=torch.zeros(5, 38, requires_grad=True), coordinates=C))


def test_two_argument_form_still_needs_its_map():
    with pytest.raises(TypeError):
        _student()(torch.zeros(5, 64))
