"""Stand-in for the parts of MinkowskiEngine the reference DRIVERS touch: `from MinkowskiEngine import
SparseTensor` (run/validation.py:17, run/train.py:17 -- imported, never used by the drivers) and
`ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(model)` (run/validation.py:201-202, run/train.py:212-213).
Everything numeric that the reference does through ME (SparseTensor maths, MinkowskiConvolution, MinkowskiBatchNorm) lives
in models/affinity_module.py, which geopurify_amd.affinity_module replaces with HIP kernels."""
from enum import Enum
from types import SimpleNamespace

import torch

__version__ = "0.0-geopurify-amd-stub"


class SparseTensorQuantizationMode(Enum):
    """The members of ME's enum that this stub acts on come first; the rest exist so that passing one is a clear error."""
    NO_QUANTIZATION = 0
    RANDOM_SUBSAMPLE = 1
    UNWEIGHTED_AVERAGE = 2
    UNWEIGHTED_SUM = 3
    MAX_POOL = 4
    SPLAT_LINEAR_INTERPOLATION = 5


class SparseTensor:
    """`.F` features [N,C], `.C` int32 coordinates [N,4] (batch index in column 0).

    Without `quantization_mode`, or with NO_QUANTIZATION, this is a data holder only: the rows are kept exactly as given and no kernel
    runs.  NOTE: real MinkowskiEngine defaults to RANDOM_SUBSAMPLE; this stub does not, because its existing callers (and
    AffinityPredictor, which rejects duplicate rows rather than merge them silently) hand it rows as they are.

    quantization_mode=UNWEIGHTED_AVERAGE / RANDOM_SUBSAMPLE merges duplicate coordinate rows on the GPU through
    geopurify_amd.sparse.quantize (mode "average" / "subsample", the subsample being the voxel's lowest row): `.C` holds the unique
    rows, `.F` one row per voxel (under autograd), and `.inverse_mapping` / `.unique_index` map points to voxels and voxels to
    points, so that `out.F[x.inverse_mapping]` takes per-voxel rows back to the points.  Any other mode: NotImplementedError."""

    def __init__(self, features=None, coordinates=None, device=None, quantization_mode=None, **kwargs):
        self.F = features if device is None or features is None else features.to(device)
        self.C = coordinates
        if quantization_mode is None or quantization_mode == SparseTensorQuantizationMode.NO_QUANTIZATION:
            return
        modes = {SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE: "average", SparseTensorQuantizationMode.RANDOM_SUBSAMPLE: "subsample"}
        if quantization_mode not in modes:
            raise NotImplementedError(f"SparseTensor: quantization_mode={getattr(quantization_mode, 'name', quantization_mode)} is not "
                                      "implemented (NO_QUANTIZATION, RANDOM_SUBSAMPLE and UNWEIGHTED_AVERAGE are)")
        from geopurify_amd import sparse
        coords = coordinates if device is None or not torch.is_tensor(coordinates) else coordinates.to(device)
        q = sparse.quantize(coords, self.F, mode=modes[quantization_mode])
        self.F, self.C = q.features, q.coordinates
        self.inverse_mapping, self.unique_index = q.inverse_mapping, q.unique_index

    @property
    def features(self):
        return self.F

    @property
    def coordinates(self):
        return self.C


def _batched_coordinates(coords, dtype=torch.int32, device=None):
    """ME.utils.batched_coordinates: floor to int32 and prepend the batch index (models/affinity_module.py:1543)."""
    out = []
    for b, c in enumerate(coords):
        ci = torch.floor(torch.as_tensor(c).float()).to(dtype)
        out.append(torch.cat([torch.full((ci.shape[0], 1), b, dtype=dtype, device=ci.device), ci], 1))
    res = torch.cat(out)
    return res if device is None else res.to(device)


def _sparse_quantize(coordinates, features=None, labels=None, ignore_label=-100, return_index=False, return_inverse=False,
                     quantization_size=None):
    """ME.utils.sparse_quantize on the GPU: coordinates [N,3] (no batch column), optionally divided by quantization_size and
    floored; returns the unique coordinates i32 [M,3], then features[index] if given, then the labels if given (ignore_label where
    two labels of a voxel differ), then the index (the lowest row of each voxel) if return_index, then the inverse map if
    return_inverse -- ME's order.  A single return value is not wrapped in a tuple.  The rows come in ascending Morton key, where
    ME's order is that of its hash map."""
    from geopurify_amd import sparse
    if not torch.is_tensor(coordinates) or coordinates.dim() != 2 or coordinates.shape[1] != 3:
        raise ValueError(f"sparse_quantize: coordinates must be [N, 3], got "
                         f"{list(coordinates.shape) if torch.is_tensor(coordinates) else type(coordinates).__name__}")
    if features is not None and (not torch.is_tensor(features) or features.dim() != 2 or features.shape[0] != coordinates.shape[0]):
        raise ValueError(f"sparse_quantize: features must be [N, D] with N = {coordinates.shape[0]} coordinate rows")
    q = sparse.quantize(torch.cat([torch.zeros_like(coordinates[:, :1]), coordinates], 1), None, labels,
                        quantization_size=quantization_size, ignore_label=ignore_label, collision="differ")
    out = [q.coordinates[:, 1:].contiguous()]
    if features is not None:
        out.append(features[q.unique_index])
    if labels is not None:
        out.append(q.labels)
    if return_index:
        out.append(q.unique_index)
    if return_inverse:
        out.append(q.inverse_mapping)
    return out[0] if len(out) == 1 else tuple(out)


utils = SimpleNamespace(batched_coordinates=_batched_coordinates, sparse_quantize=_sparse_quantize)


class MinkowskiSyncBatchNorm:
    @classmethod
    def convert_sync_batchnorm(cls, module, process_group=None):
        """Returns the module unchanged: nothing needs converting.  BatchNorm in training mode is computed by the HIP training step
        (geopurify_amd/training.py), which synchronises the batch statistics over the ranks by itself whenever torch.distributed is
        initialised with more than one rank (StudentTrainer(sync_bn=True): fp64 column sums all-reduced, sharding.sync_batch_stats) --
        what the reference obtains from this call (run/train.py:212-213)."""
        return module
