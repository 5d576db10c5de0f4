"""The reference's Gaussian density field on HIP (``csrc/density.hip``): exact k-nearest neighbours over the means, the density of
``get_density`` and the analytic normal of ``get_density_grad`` (dn_splatter/dn_model.py:1061-1135, :1449-1494), at arbitrary samples
or on the lattice of the marching-cubes exporter (export_mesh.py:700-820).

Where the reference runs sklearn's kd-tree on the CPU per batch (``knn_sk``, fed by ``.cpu().numpy()`` copies of all the means and of
the batch) and then gathers [M,16,3,3] matrices to produce M floats, this module keeps a uniform-grid index and one 16-float record per
Gaussian on the device and evaluates a sample in one thread: ``dnsplat_knn_build`` / ``dnsplat_density_pack`` once per snapshot,
``dnsplat_knn_query`` / ``dnsplat_density_eval`` per call, nothing read on the host.

  * ``knn`` / ``build_index``: the search alone; ranks in float64 like sklearn, index-exact; ``skip=1`` is ``knn_sk``'s dropped column;
  * ``GaussianDensityField``: a snapshot of (means, scales, quats, opacities) with ``closest`` / ``density`` / ``density_grad`` / ``volume``;
  * ``density_volume``: the grid, mask and fill of ``MarchingCubesMesh.main``;
  * ``install_density(model)``: the three methods with the reference's signatures, bound onto a model.

``torch_density`` is the PyTorch restatement.  There is no CPU fallback."""
from __future__ import annotations

import ctypes
import types
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import DnsplatError
from ._ops import _density_args, _f32c, _need_gpu, _ptr, _stream
from .torch_density import KNN, SKIP
from .torch_export import within

MAX_K = 32              # include/dnsplat.h DNSPLAT_KNN_MAX_K
RECORD_FLOATS = 16


def _points(t: Tensor, name: str) -> Tensor:
    t = _f32c(t.detach(), name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n,3], got {tuple(t.shape)}")
    return t


def _check_k(N: int, k: int, skip: int) -> None:
    if k < 1 or skip < 0:
        raise ValueError(f"k must be >= 1 and skip >= 0, got k = {k}, skip = {skip}")
    if k + skip > MAX_K:
        raise ValueError(f"k + skip = {k + skip} exceeds {MAX_K}")
    if k + skip > N:
        raise ValueError(f"k + skip = {k + skip} neighbours asked of {N} points (sklearn: n_neighbors <= n_samples_fit)")


class KnnIndex:
    """The uniform-grid index of ``points`` [N,3] (a snapshot: the sorted copy lives in the buffer)."""

    def __init__(self, points: Tensor):
        points = _points(points, "points")
        self.N = points.shape[0]
        if self.N < 1:
            raise ValueError("an index needs at least one point")
        L = _lib.lib()
        self.buffer = torch.empty(L.dnsplat_knn_index_bytes(self.N) // 8, dtype=torch.int64, device=points.device)
        _lib.run("dnsplat_knn_build", L.dnsplat_knn_build, self.N, _ptr(points), _ptr(self.buffer), _stream())
        self._points = None

    @property
    def device(self):
        return self.buffer.device

    def points(self) -> Tensor:
        """float32 [N,3]: the points the index was built over, in their own order and bit for bit, recovered from the sorted copy the
        buffer holds (``dnsplat_knn_points``); kept after the first call.  The mesh alignment reads its targets from it."""
        if self._points is None:
            out = torch.empty(self.N, 3, dtype=torch.float32, device=self.device)
            L = _lib.lib()
            _lib.run("dnsplat_knn_points", L.dnsplat_knn_points, self.N, _ptr(self.buffer), _ptr(out), _stream())
            self._points = out
        return self._points

    def query(self, queries: Tensor, k: int, skip: int = 0, return_d2: bool = False):
        """int32 [M,k]: ranks ``skip .. skip + k - 1`` by (d², index), d² in float64; with ``return_d2`` also d² as float32 [M,k]."""
        queries = _points(queries, "queries")
        _check_k(self.N, k, skip)
        M = queries.shape[0]
        idx = torch.empty(M, k, dtype=torch.int32, device=queries.device)
        d2 = torch.empty(M, k, dtype=torch.float32, device=queries.device) if return_d2 else None
        L = _lib.lib()
        _lib.run("dnsplat_knn_query", L.dnsplat_knn_query, self.N, _ptr(self.buffer), M, _ptr(queries), int(k), int(skip), _ptr(idx), _ptr(d2),
                 _stream())
        return (idx, d2) if return_d2 else idx


def build_index(points: Tensor) -> KnnIndex:
    return KnnIndex(points)


def knn(points, queries: Tensor, k: int, skip: int = 0, return_d2: bool = False):
    """The ``k`` nearest of ``points`` ([N,3], or a ``KnnIndex``) to every query, after the first ``skip``: int32 [M,k] (and d² float32).
    ``knn(means, means, 3, skip=1)`` is the 3-NN of the scale initialisation; ``knn(means, samples, 16, skip=1)`` is ``knn_sk``."""
    index = points if isinstance(points, KnnIndex) else KnnIndex(points)
    return index.query(queries, k, skip, return_d2)


class GaussianDensityField:
    """A snapshot of the Gaussians' raw parameters as the model stores them — ``means`` [N,3], ``scales`` [N,3] (log), ``quats`` [N,4]
    (wxyz, any norm), ``opacities`` [N,1] or [N] (logit) — that owns the index and the records."""

    def __init__(self, means: Tensor, scales: Tensor, quats: Tensor, opacities: Tensor):
        means = _points(means, "means")
        N = means.shape[0]
        scales, quats, opacities = _f32c(scales.detach(), "scales"), _f32c(quats.detach(), "quats"), _f32c(opacities.detach(), "opacities")
        if tuple(scales.shape) != (N, 3) or tuple(quats.shape) != (N, 4) or opacities.numel() != N:
            raise ValueError(f"for {N} means: scales [N,3], quats [N,4], opacities [N,1]; got {tuple(scales.shape)}, {tuple(quats.shape)}, "
                             f"{tuple(opacities.shape)}")
        self.N = N
        # the level-set ray step reads them per closest Gaussian.  Copies, as the records are: the field is a snapshot, and an optimiser
        # step on the model's parameters must not leave the ray step with other scales than the records were packed from
        self.scales_log, self.quats = scales.clone(), quats.clone()
        self.index = KnnIndex(means)
        self.records = torch.empty(N, RECORD_FLOATS, dtype=torch.float32, device=means.device)
        L = _lib.lib()
        _lib.run("dnsplat_density_pack", L.dnsplat_density_pack, N, _ptr(means), _ptr(scales), _ptr(quats), _ptr(opacities), _ptr(self.records),
                 _stream())

    @property
    def device(self):
        return self.records.device

    def closest(self, samples: Tensor) -> Tensor:
        """``get_closest_gaussians``: int64 [M,16] — ranks 1 .. 16 of 17, as ``knn_sk`` returns them for any samples."""
        return self.index.query(samples, KNN, SKIP).to(torch.int64)

    def _eval(self, samples, lattice, mask, fill, neighbors, k, skip, num_closest, want_density, want_normals):
        dev = self.device
        if neighbors is not None:
            _need_gpu(neighbors, "closest_gaussians")
            if neighbors.dtype not in (torch.int32, torch.int64) or neighbors.dim() != 2 or neighbors.shape[0] != samples.shape[0]:
                raise TypeError(f"closest_gaussians must be an int32 or int64 [M,k] tensor, got {neighbors.dtype} {tuple(neighbors.shape)}")
            neighbors = neighbors.contiguous()
            k, skip = neighbors.shape[1], 0
            if k < 1:
                raise ValueError("closest_gaussians has no columns")
        else:
            _check_k(self.N, k, skip)
        if num_closest is not None and not 1 <= num_closest:
            raise ValueError(f"num_closest_gaussians must be >= 1, got {num_closest}")
        nc = 0 if num_closest is None else min(int(num_closest), k)
        rows = samples.shape[0] if samples is not None else lattice[0].numel() * lattice[1].numel() * lattice[2].numel()
        density = torch.empty(rows, dtype=torch.float32, device=dev) if want_density else None
        normals = torch.empty(rows, 3, dtype=torch.float32, device=dev) if want_normals else None
        a = _density_args(self.N, self.index.buffer, self.records, samples, lattice, mask, float(fill), neighbors, int(k), int(skip), nc,
                          density, normals)
        L = _lib.lib()
        _lib.run("dnsplat_density_eval", L.dnsplat_density_eval, ctypes.byref(a), _stream())
        return density, normals

    def density(self, samples: Tensor, closest_gaussians: Optional[Tensor] = None) -> Tensor:
        """``get_density(samples, closest_gaussians)``: float32 [M].  Without ``closest_gaussians`` the search runs inside the kernel."""
        return self._eval(_points(samples, "samples"), None, None, 0.0, closest_gaussians, KNN, SKIP, None, True, False)[0]

    def density_grad(self, samples: Tensor, num_closest_gaussians: Optional[int] = None, closest_gaussians: Optional[Tensor] = None) -> Tensor:
        """``get_density_grad``: float32 [M,3], minus the normalised density gradient over the first ``num_closest_gaussians``."""
        k = KNN if num_closest_gaussians is None else max(1, min(KNN, int(num_closest_gaussians)))
        return self._eval(_points(samples, "samples"), None, None, 0.0, closest_gaussians, k, SKIP, num_closest_gaussians, False, True)[1]

    def volume(self, X: Tensor, Y: Tensor, Z: Tensor, mask: Optional[Tensor] = None, fill: float = 0.0) -> Tensor:
        """float32 [Rx,Ry,Rz]: ``density`` at (X[i], Y[j], Z[k]) in ``meshgrid(..., indexing="ij")`` order; where ``mask`` (bool
        [Rx,Ry,Rz]) is False the value is ``fill`` and nothing is evaluated."""
        axes = []
        for name, t in (("X", X), ("Y", Y), ("Z", Z)):
            t = _f32c(t, name)
            if t.dim() != 1 or t.numel() < 1:
                raise ValueError(f"{name} must be a non-empty 1-D tensor, got {tuple(t.shape)}")
            axes.append(t)
        shape = tuple(t.numel() for t in axes)
        if mask is not None:
            _need_gpu(mask, "mask")
            if mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != shape[0] * shape[1] * shape[2]:
                raise ValueError(f"mask must be a bool tensor of {shape}, got {mask.dtype} {tuple(mask.shape)}")
            mask = mask.reshape(shape).contiguous()
        return self._eval(None, tuple(axes), mask, fill, None, KNN, SKIP, None, True, False)[0].reshape(shape)


def density_volume(field: GaussianDensityField, resolution: int, radius: float, crop_box=None) -> Tensor:
    """export_mesh.py:740-773: the [R,R,R] lattice ``linspace(-1, 1, R) * radius`` per axis, the density inside ``crop_box`` (anything
    with ``OrientedBox``'s R, T, S; ``torch_export.within``), -1e6 outside it; without a box every point is evaluated."""
    X = torch.linspace(-1, 1, int(resolution), device=field.device) * radius
    mask = None
    if crop_box is not None:
        xx, yy, zz = torch.meshgrid(X, X, X, indexing="ij")
        mask = within(crop_box, torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3)).reshape(xx.shape)
    return field.volume(X, X, X, mask=mask, fill=-1e6)


_FIELD = "_dnsplat_density_field"
_PARAMS = ("means", "scales", "quats", "opacities")


def _model_field(model) -> GaussianDensityField:
    """The snapshot of ``model``'s parameters, rebuilt when one of them was written in place (``_version``), replaced or resized."""
    tensors = [getattr(model, name) for name in _PARAMS]
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors)
    cached = model.__dict__.get(_FIELD)
    if cached is None or cached[0] != key:
        cached = (key, GaussianDensityField(*(t.data if isinstance(t, torch.nn.Parameter) else t for t in tensors)))
        object.__setattr__(model, _FIELD, cached)
    return cached[1]


def install_density(model):
    """Binds ``get_closest_gaussians(samples)``, ``get_density(sdf_samples, closest_gaussians=None, vis_indices=None)`` and
    ``get_density_grad(samples, num_closest_gaussians=None, closest_gaussians=None)`` — the reference's signatures — onto ``model``
    (anything with ``means``, ``scales``, ``quats``, ``opacities``).  They run on a ``GaussianDensityField`` snapshot that is rebuilt
    when a parameter's ``_version`` or shape changes.  Returns the names bound."""
    def get_closest_gaussians(self, samples):
        return _model_field(self).closest(samples.to(_model_field(self).device))

    def get_density(self, sdf_samples, closest_gaussians=None, vis_indices=None):
        return _model_field(self).density(sdf_samples, closest_gaussians)

    def get_density_grad(self, samples, num_closest_gaussians=None, closest_gaussians=None):
        if num_closest_gaussians is not None:
            assert num_closest_gaussians >= 1
        return _model_field(self).density_grad(samples, num_closest_gaussians, closest_gaussians)

    bound = []
    for fn in (get_closest_gaussians, get_density, get_density_grad):
        object.__setattr__(model, fn.__name__, types.MethodType(torch.no_grad()(fn), model))
        bound.append(fn.__name__)
    return bound
