"""Host-side mirror of the reference's layer interface for the accelerated path.

Same class names, constructor arguments, parameters / buffers (names, shapes, dtypes) and
``forward(p_pc_in, p_pc_out, p_in_features, p_neighborhood)`` signature as

  * ``PreProcessModule``          point_cloud_lib/layers/PreProcessModule.py:3-53
  * ``IConvLayer`` / ``IConvLayerFactory``   point_cloud_lib/layers/IConvLayer.py:8-160
  * ``PNEConvLayerRotEquiv`` / ``PNEConvLayerRotEquivFactory``
                                  point_cloud_lib/layers/PNEConvLayerRotEquiv.py:49-281
    (parameter creation: point_cloud_lib/layers/PNEConvLayer.py:79-88, 151-158)

so that ``load_state_dict`` of a reference checkpoint works and the model code that calls convs
through the factory runs unchanged.  The convolution itself is one call into the HIP library
(``ops.SE3ConvFunction``); nothing E'-sized is built in Python.
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import ops


class PreProcessModule(torch.nn.Module):
    """Module with a "pre-process" mode that is switched on/off recursively for all
    PreProcessModule children, including those nested in ModuleLists."""

    def __init__(self):
        self.pre_process_ = False
        super().__init__()

    def _set_children(self, module, flag: bool):
        for child in module.children():
            if isinstance(child, PreProcessModule):
                child.start_pre_process() if flag else child.end_pre_process()
            elif isinstance(child, torch.nn.ModuleList):
                self._set_children(child, flag)

    def start_pre_process(self):
        self.pre_process_ = True
        self._set_children(self, True)

    def end_pre_process(self):
        self.pre_process_ = False
        self._set_children(self, False)


class IConvLayer(PreProcessModule, ABC):
    """Interface of a point convolution: owns the two EMA normalisers (both start at 0)."""

    def __init__(self, p_dims, p_in_features, p_out_features):
        super().__init__()
        self.dims_ = p_dims
        self.feat_input_size_ = p_in_features
        self.feat_output_size_ = p_out_features
        self.register_buffer("norm_neigh_dist_", torch.tensor(0, dtype=torch.float32))
        self.register_buffer("norm_num_neighs_", torch.tensor(0, dtype=torch.float32))

    @abstractmethod
    def __compute_convolution__(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        pass

    def forward(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        if self.pre_process_:
            # (inference_mode(False): a buffer rebound inside a caller's inference_mode block would be an inference tensor,
            # which autograd refuses to save in the next training step)
            with torch.no_grad(), torch.inference_mode(False):
                # IConvLayer.py:76-97.  Ball query: 1/radius.  (kNN neighbourhoods use half the
                # inverse mean edge length.)  nu uses point-level M / E.
                radius = getattr(p_neighborhood, "radius_", None)
                if radius is not None:
                    new_dist = torch.tensor(1.0 / radius, dtype=torch.float32)
                else:
                    nb = p_neighborhood.neighbors_
                    diff = p_pc_in.pts_[nb[:, 1].long(), :] - p_pc_out.pts_[nb[:, 0].long(), :]
                    mean_len = torch.mean(torch.sqrt(torch.sum(diff ** 2, -1))).item()
                    new_dist = torch.tensor(1.0 / (2.0 * mean_len), dtype=torch.float32)
                self.norm_neigh_dist_ = 0.9 * self.norm_neigh_dist_ + 0.1 * new_dist
                n_edges = p_neighborhood.num_edges() if hasattr(p_neighborhood, "num_edges") else \
                    p_neighborhood.neighbors_.shape[0]
                new_num = torch.tensor(p_neighborhood.start_ids_.shape[0] / n_edges, dtype=torch.float32)
                self.norm_num_neighs_ = 0.9 * self.norm_num_neighs_ + 0.1 * new_num
        return self.__compute_convolution__(p_pc_in, p_pc_out, p_in_features, p_neighborhood)


class IConvLayerFactory(ABC):
    def __init__(self, p_dims):
        super().__init__()
        self.dims_ = p_dims
        self.conv_list_ = []

    def update_parameters(self, **kwargs):
        pass

    @abstractmethod
    def __create_conv_layer_imp__(self, p_in_features, p_out_features):
        pass

    def create_conv_layer(self, p_in_features, p_out_features):
        conv = self.__create_conv_layer_imp__(p_in_features, p_out_features)
        self.conv_list_.append(conv)
        return conv


def _geometry_of(p_pc_in, p_pc_out, p_neighborhood) -> ops.ConvGeometry:
    """int32/fp32 view of the clouds + neighbourhood, cached on the neighbourhood object (it also
    carries the lazily built source-major edge list used by backward)."""
    cache = getattr(p_neighborhood, "_se3_geom", None)
    nb32 = getattr(p_neighborhood, "neighbors_i32_", None)  # the library's own list when it built the neighbourhood
    if nb32 is None:
        nb32 = p_neighborhood.neighbors_
    key = (id(p_pc_in), id(p_pc_out), nb32.data_ptr(), p_pc_in.local_frames_.data_ptr(),
           p_pc_out.local_frames_.data_ptr(), p_pc_in.pts_.data_ptr(), p_pc_out.pts_.data_ptr())
    if cache is not None and cache[0] == key:
        _refresh_copies(cache[1], cache[2])
        return cache[1]
    geom = ops.ConvGeometry.build(p_pc_in.pts_, p_pc_out.pts_, p_pc_in.local_frames_, p_pc_out.local_frames_,
                                  nb32, p_neighborhood.start_ids_,
                                  symmetric=bool(getattr(p_neighborhood, "symmetric_", False)) and p_pc_in is p_pc_out)
    geom.edge_info = getattr(p_neighborhood, "edge_info_", None)
    geom.bounded = geom.edge_info is not None
    if geom.symmetric:
        geom.sources = getattr(p_neighborhood, "sources_i32_", None)
    geom.source_major_fn = getattr(p_neighborhood, "source_major", None)
    # the clouds' packed geometry records: built once per cloud by whichever call meets them first, shared by every other
    geom.records_in = ops.prepared_records(p_pc_in)
    geom.records_out = geom.records_in if p_pc_out is p_pc_in else ops.prepared_records(p_pc_out)
    sources = ((p_pc_in.pts_, geom.pts_in), (p_pc_out.pts_, geom.pts_out), (p_pc_in.local_frames_, geom.frames_in),
               (p_pc_out.local_frames_, geom.frames_out))
    # the tensors the geometry holds as converted COPIES (float64 points, non-contiguous frames, ...), with the version of
    # the cloud's tensor they were made from: an in-place update of the cloud must reach them
    copies = [[src, held, ops.version_key(src)] for src, held in sources if held.data_ptr() != src.data_ptr()]
    try:
        p_neighborhood._se3_geom = (key, geom, copies)
    except AttributeError:
        pass
    return geom


def _refresh_copies(geom: ops.ConvGeometry, copies) -> None:
    """Converts again, in place, what the cached geometry holds as a copy of a cloud tensor that has changed since (and,
    inside a HIP graph capture, every such copy: a replay must convert what the cloud holds then).  The copy's own version
    moves with it, so the records bound to it are rebuilt too."""
    if not copies:
        return
    capturing = geom.pts_out.is_cuda and torch.cuda.is_current_stream_capturing()
    for entry in copies:
        src, held, version = entry
        if capturing or ops.version_key(src) != version:
            held.copy_(src.detach().reshape(held.shape))
            entry[2] = ops.version_key(src)


_ACTIVATIONS = {"mlp_gelu": torch.nn.functional.gelu, "mlp_relu": torch.relu, "mlp_sin": torch.sin, "mlp_linear": (lambda t: t),
                "mlp_softmax": (lambda t: torch.softmax(t, dim=-1))}  # PNEConvLayer.py:91-100 besides mlp_gelu


def _conv_materialised(feat, axes, biases, weights, geom, rho, nu, act, rel_rot="6D"):
    """The reference's own formulation (PNEConvLayerRotEquiv.py:199-216) on the library's API-parity ops, for the
    kernel-MLP activations the fused operator does not implement (no *_rot configuration uses them): descriptors
    materialised by ``se3_rot_tensors``, ``act(desc @ A + beta)`` and the contraction in torch, the aggregation
    through ``FeatBasisProj``.  Memory and time of the reference's path (E'-sized tensors), not of the fused one."""
    if getattr(geom, "bounded", False):
        raise NotImplementedError("a capacity-bounded neighbourhood (rows past the edge count are unset) cannot feed "
                                  "the materialised path: build the neighbourhood without p_capacity")
    desc, neighbs, ends = ops.rot_tensors(geom, rho, rel_rot)
    phi = act(torch.matmul(desc, axes) + biases)
    t = ops.FeatBasisProj.apply(phi, feat, neighbs, ends)
    out = torch.einsum("nik,iko->no", t, weights)
    return out / geom.frames_in.shape[1] * nu


_REL_ROT_DIMS = {"6D": 9, "matrix": 12, "quaternion": 7}  # p_rel_rot -> p_dims (RotationFunctions.py:593-600)
def _conv_any_num_basis(feat, axes, biases, weights, geom, rho, nu):
    """The fused operator for any number of basis functions K.  The MFMA kernels work on 32 basis functions; the library
    itself runs other K as slices of 32 (the sum over k is separable; a short slice is padded with basis functions whose
    conv weights are zero: exact) -- `se3conv_fwd` / `se3conv_bwd` with `num_basis != 32`, include/se3conv.h.  The
    reference's CUDA op accepts K in {8, 16, 32, 64} (feat_basis_utils.cuh:35-41); every shipped configuration uses 32."""
    return ops.SE3ConvFunction.apply(feat, axes, biases, weights, geom, rho, nu)


class PNEConvLayerRotEquiv(IConvLayer):
    """SE(3)-equivariant continuous point convolution (reference class of the same name).

    Differences that are deliberate (DESIGN.md "Quirks"):
      * the output always has ``N_out * F_out`` rows (the reference drops trailing rows that have
        no neighbours because its degree histogram has no ``dim_size``, :111-114);
      * there is no rot-tensor cache to hash (no D2H copy + SHA-256 per call, :71): the descriptors
        are recomputed inside the kernel.  ``rot_tensor_cache`` / ``empty_rot_tenors_cache`` /
        ``get_rot_tenors`` are kept for API compatibility.

    Padded clouds (``Pointcloud(..., p_n_valid=)``, a neighbourhood built with ``p_capacity``) need nothing of the operator:
    an absent sample has no edges, so its output rows are exactly 0, and an absent source has none either, so its ``dX``
    rows are exactly 0.  The caller's obligation: the feature rows of absent points hold FINITE values (the weight gradient
    is formed as ``sum_p f[p] * U[p]``, and ``U[p] = 0`` does not survive a NaN); which finite values changes no result.
    ``pre_process_`` reads edge counts on the host: keep it off in a captured step.
    """

    rot_tensor_cache = {}
    rel_rot_type = "6D"

    @staticmethod
    def empty_rot_tenors_cache():
        PNEConvLayerRotEquiv.rot_tensor_cache = {}

    @staticmethod
    def get_rot_tenors(p_pc_in, p_pc_out, p_neighborhood, radius):
        """Materialised rot tensors with the reference's dict keys (computed on the GPU, not
        cached by content hash).  ``radius`` is the layer's ``norm_neigh_dist_`` like in the reference; the relative
        rotation comes in the class-level ``rel_rot_type`` representation, as there."""
        with torch.no_grad():
            geom = _geometry_of(p_pc_in, p_pc_out, p_neighborhood)
            desc, neighbs, ends = ops.rot_tensors(geom, radius, PNEConvLayerRotEquiv.rel_rot_type)
            rel_pt = (geom.pts_in[geom.neighbors[:, 1].long()] - geom.pts_out[geom.neighbors[:, 0].long()]) * \
                torch.as_tensor(radius, dtype=torch.float32, device=geom.pts_in.device)
            return {"tensor": rel_pt, "rel_pts_rel_orient": desc, "neighbs": neighbs.to(torch.int64),
                    "neighbs_start_ids": ends}

    def __init__(self, p_dims, p_in_features, p_out_features, p_num_basis, p_pne_type):
        super().__init__(p_dims, p_in_features, p_out_features)
        self.num_basis_ = p_num_basis
        self.pne_type_ = p_pne_type
        self.aggregation_ = "add"
        if "kp" in p_pne_type:
            # same behaviour as the reference, which raises at call time (:221-222)
            self.proj_axes_ = None
        if "mlp" in p_pne_type:
            bound = math.sqrt(1.0 / p_dims)
            self.proj_axes_ = torch.nn.Parameter(torch.empty(p_dims, p_num_basis).uniform_(-bound, bound))
            self.proj_biases_ = torch.nn.Parameter(torch.zeros((p_num_basis,), dtype=torch.float32))
        bound = math.sqrt(1.0 / (p_in_features * p_num_basis))
        self.conv_weights_ = torch.nn.Parameter(
            torch.empty(p_in_features, p_num_basis, p_out_features).uniform_(-bound, bound))

    def __compute_convolution__(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        if "mlp" in self.pne_type_:
            rel_rot = PNEConvLayerRotEquiv.rel_rot_type  # class attribute set by the last-created factory (:278), as the reference
            if rel_rot not in _REL_ROT_DIMS:
                raise ValueError(f"rel_rot_type {rel_rot!r}: expected one of {sorted(_REL_ROT_DIMS)}")
            if self.dims_ != _REL_ROT_DIMS[rel_rot]:
                raise ValueError(f"p_dims = {self.dims_} but the '{rel_rot}' descriptor has {_REL_ROT_DIMS[rel_rot]} entries")
            if self.pne_type_ not in _ACTIVATIONS:
                raise Exception(f"unknown pne type {self.pne_type_}")
            geom = _geometry_of(p_pc_in, p_pc_out, p_neighborhood)
            if self.pne_type_ != "mlp_gelu" or rel_rot != "6D":
                # activations / relative-rotation representations no *_rot configuration uses: the reference's own
                # materialised formulation on the library's API-parity ops
                return _conv_materialised(p_in_features, self.proj_axes_, self.proj_biases_, self.conv_weights_, geom,
                                          self.norm_neigh_dist_, self.norm_num_neighs_, _ACTIVATIONS[self.pne_type_], rel_rot)
            return _conv_any_num_basis(p_in_features, self.proj_axes_, self.proj_biases_, self.conv_weights_, geom,
                                       self.norm_neigh_dist_, self.norm_num_neighs_)
        elif "kp" in self.pne_type_:
            raise Exception("KPNE convolution not implemeted yet for Rot Equiv.")
        raise Exception(f"unknown pne type {self.pne_type_}")


def _identity_frames(pc) -> torch.Tensor:
    """``[N,1,9]`` identity frames of a plain Pointcloud, cached on it."""
    fr = getattr(pc, "_se3_identity_frames", None)
    if fr is None or fr.shape[0] != pc.pts_.shape[0] or fr.device != pc.pts_.device:
        fr = torch.eye(3, dtype=torch.float32, device=pc.pts_.device).reshape(1, 1, 9).repeat(pc.pts_.shape[0], 1, 1)
        try:
            pc._se3_identity_frames = fr
        except AttributeError:
            pass
    return fr


class _IdentityFramed(object):
    """View of a plain Pointcloud with one identity frame per point (what the fused operator reads)."""

    def __init__(self, pc):
        self.pts_ = pc.pts_
        self.local_frames_ = _identity_frames(pc)
        self.n_frames_ = 1


def create_pts_icosphere(subdiv, return_faces=False):
    """The vertices ``[V,3]`` (float64, on the unit sphere) of an icosahedron whose triangles are split ``subdiv`` times:
    12 vertices for 0, 42 for 1, ``10 * 4**subdiv + 2`` in general.  Vertices and order are those of the reference's function
    of the same name (tests/golden/icosphere.npz holds its output), the construction is this package's own:

      * two poles on the y axis and two rings of five at ``y = +-1/sqrt(5)``, 72 degrees apart in azimuth (measured from +z
        towards +x), the lower ring turned by 36 degrees against the upper;
      * the twenty faces in four bands of five -- the fan of the upper pole in ascending azimuth, the triangles that hang
        from the upper ring in descending azimuth, the fan of the lower pole in descending azimuth, the triangles that stand
        on the lower ring;
      * a split puts the midpoint of every edge on the sphere, once per edge, in the order the faces meet their edges."""
    s5 = math.sqrt(5.0)

    def ring(y, deg):
        a = math.radians(deg)
        return (2.0 / s5 * math.sin(a), y, 2.0 / s5 * math.cos(a))

    up = {d: ring(1.0 / s5, d) for d in range(0, 360, 72)}       # azimuth -> vertex of the upper ring
    low = {d: ring(-1.0 / s5, d) for d in range(36, 360, 72)}
    top, bottom = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
    verts = [top, up[0], low[180], bottom, low[252], up[288], low[108], up[72], low[36], low[324], up[144], up[216]]
    at = {v: i for i, v in enumerate(verts)}
    faces = [[at[top], at[up[(216 + 72 * i) % 360]], at[up[(288 + 72 * i) % 360]]] for i in range(5)]
    faces += [[at[up[a % 360]], at[up[(a - 72) % 360]], at[low[(a - 36) % 360]]] for a in range(360, 0, -72)]
    faces += [[at[bottom], at[low[a % 360]], at[low[(a - 72) % 360]]] for a in range(324, -36, -72)]
    stand = [[at[low[a % 360]], at[low[(a + 72) % 360]], at[up[(a + 36) % 360]]] for a in range(252, -108, -72)]
    stand[0] = stand[0][2:] + stand[0][:2]     # (the first of them is listed from its upper vertex)
    faces += stand
    verts = [list(v) for v in verts]
    for _ in range(int(subdiv)):
        cut = {}

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cut:
                m = [(a + b) / 2 for a, b in zip(verts[i], verts[j])]
                n = math.sqrt(sum(c * c for c in m))
                verts.append([c / n for c in m])
                cut[key] = len(verts) - 1
            return cut[key]

        split = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            split += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        faces = split
    v = np.array(verts, dtype=np.float64)
    return (v, np.array(faces)) if return_faces else v


def _random_rotation() -> torch.Tensor:
    """A rotation matrix ``[3,3]`` (float64) drawn uniformly: a unit quaternion from four normal variates."""
    q = torch.randn(4, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


# PNEConvLayer.py:104-134: (scale of the kernel points, sigma per correlation function) of the single and the double set
_KP_SETS = {False: (0.6, {"linear": 0.4, "gauss": 0.3, "box": 1.0}), True: (0.35, {"linear": 0.2, "gauss": 0.16, "box": 1.0})}
PNE_TYPES = tuple(_ACTIVATIONS) + tuple(f"kp_{c}{d}" for d in ("", "_double") for c in ("linear", "gauss", "box"))
_FEAT_BASIS_K = (8, 16, 32, 64)  # the K of se3_feat_basis_proj (the reference's CUDA op: feat_basis_utils.cuh:35-41)


def kernel_points(p_pne_type: str):
    """The unrotated kernel points ``[J,3]`` (float64) of a ``kp_*`` type: the icosahedron and the origin, scaled by 0.6
    (J = 13), or for ``*_double`` the icosahedron at 0.35, its first split at 0.7 and the origin (J = 55)."""
    double = "double" in p_pne_type
    scale = _KP_SETS[double][0]
    sets = [create_pts_icosphere(0) * scale] + ([create_pts_icosphere(1) * scale * 2] if double else [])
    return np.concatenate(sets + [np.zeros((1, 3))])


class PNEConvLayer(IConvLayer):
    """The reference's non-equivariant continuous convolution (``layers/PNEConvLayer.py:47-229``, scope row f-4):

        add:  out[s,o] = nu * sum_{(s,p) in E} sum_k sum_i phi(rho (x_p - y_s))_k * f[p,i] * W[i,k,o]
        max:  out[s,o] = nu * max_{(s,p) in E} sum_k sum_i phi(rho (x_p - y_s))_k * f[p,i] * W[i,k,o]      (0 without an edge)

    with every embedding ``phi`` of the reference (``PNE_TYPES``): the kernel MLP ``act(r . A + beta)`` with five activations,
    and the kernel-point embeddings ``corr(|r - kp_j| / sigma) . A + beta`` (KPConv-style; ``kernel_pts_ [J,3]`` is a buffer,
    randomly rotated once at construction).  Parameter / buffer names and shapes are the reference's (``proj_axes_ [3,K]`` or
    ``[J,K]``, ``proj_biases_ [K]``, ``conv_weights_ [C_in,K,C_out]``).

    ``mlp_gelu`` with ``add`` runs through the same HIP operator as the equivariant layer: with one identity frame per point
    the 9-D descriptor of the fused kernel is ``[rho (x_p - y_s), 1,0,0, 0,1,0]``, so the ``[3,K]`` projection axes are padded
    with six zero rows (whose gradient rows are dropped by autograd's ``cat``).  Every other ``add`` configuration is
    ``ops.PneEmbed -> ops.FeatBasisProj -> einsum`` (K in {8, 16, 32, 64}, as that operator); ``max`` is ``ops.PneEmbed``, one dense
    product ``G = f @ W`` and ``ops.NeighConvMax``.  The output always has one row per output point (DESIGN.md "Quirks").
    Capacity-bounded neighbourhoods (``p_capacity``) feed the fused path only.
    """

    def __init__(self, p_dims, p_in_features, p_out_features, p_num_basis, p_pne_type, p_aggregation="add"):
        super().__init__(p_dims, p_in_features, p_out_features)
        self.num_basis_ = p_num_basis
        self.pne_type_ = p_pne_type
        self.aggregation_ = p_aggregation
        if p_dims != 3:
            raise NotImplementedError("PNEConvLayer on the HIP library: 3-D points")
        if p_pne_type not in PNE_TYPES:
            raise ValueError(f"unknown pne type {p_pne_type!r}: expected one of {PNE_TYPES}")
        if p_aggregation not in ("add", "max"):
            raise ValueError(f"unknown aggregation {p_aggregation!r}: expected 'add' or 'max'")
        self.fused_ = p_pne_type == "mlp_gelu" and p_aggregation == "add"
        if p_aggregation == "add" and not self.fused_ and p_num_basis not in _FEAT_BASIS_K:
            raise ValueError(f"PNEConvLayer('{p_pne_type}', 'add') aggregates through FeatBasisProj, which takes a number of basis "
                             f"functions in {set(_FEAT_BASIS_K)}, not {p_num_basis}")
        if "kp" in p_pne_type:
            # the correlation function by substring: the reference's `if` chain (:195-200) compares whole names and leaves
            # it unset for the *_double types (DESIGN.md "Quirks")
            corr = next(c for c in ("linear", "gauss", "box") if c in p_pne_type)
            self.embed_kind_ = "kp_" + corr
            self.kp_sigma_ = _KP_SETS["double" in p_pne_type][1][corr]
            kp = torch.from_numpy(kernel_points(p_pne_type)) @ _random_rotation()
            self.register_buffer("kernel_pts_", kp.to(torch.float32))
            n_in = kp.shape[0]
        else:
            self.embed_kind_ = p_pne_type
            n_in = p_dims
        bound = math.sqrt(1.0 / n_in)
        self.proj_axes_ = torch.nn.Parameter(torch.empty(n_in, p_num_basis).uniform_(-bound, bound))
        self.proj_biases_ = torch.nn.Parameter(torch.zeros((p_num_basis,), dtype=torch.float32))
        bound = math.sqrt(1.0 / (p_in_features * p_num_basis))
        self.conv_weights_ = torch.nn.Parameter(
            torch.empty(p_in_features, p_num_basis, p_out_features).uniform_(-bound, bound))

    def _conv_embedded(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        """Every configuration but ``mlp_gelu`` + ``add``: the embedding of the edges, then the aggregation."""
        if getattr(p_neighborhood, "edge_info_", None) is not None:
            raise NotImplementedError("a capacity-bounded neighbourhood (rows past the edge count are unset) cannot feed "
                                      "the materialised path: build the neighbourhood without p_capacity")
        nb32 = getattr(p_neighborhood, "neighbors_i32_", None)
        if nb32 is None:
            nb32 = p_neighborhood.neighbors_
        phi = ops.PneEmbed.apply(p_pc_in.pts_, p_pc_out.pts_, nb32, self.proj_axes_, self.proj_biases_, self.norm_neigh_dist_,
                                 self.embed_kind_, getattr(self, "kernel_pts_", None), getattr(self, "kp_sigma_", 0.0))
        if self.aggregation_ == "add":
            t = ops.FeatBasisProj.apply(phi, p_in_features, nb32, p_neighborhood.start_ids_)
            out = torch.einsum("nik,iko->no", t, self.conv_weights_)
        else:
            c_in, k, c_out = self.conv_weights_.shape
            g = torch.matmul(p_in_features, self.conv_weights_.reshape(c_in, k * c_out)).reshape(-1, k, c_out)
            out, _ = ops.NeighConvMax.apply(phi, g, nb32, p_neighborhood.start_ids_, p_in_features.shape[0], p_neighborhood)
        return out * self.norm_num_neighs_

    def __compute_convolution__(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        if not self.fused_:
            return self._conv_embedded(p_pc_in, p_pc_out, p_in_features, p_neighborhood)
        pc_in = _IdentityFramed(p_pc_in)
        pc_out = pc_in if p_pc_out is p_pc_in else _IdentityFramed(p_pc_out)
        cache = getattr(p_neighborhood, "_se3_geom_plain", None)
        nb32 = getattr(p_neighborhood, "neighbors_i32_", None)
        if nb32 is None:
            nb32 = p_neighborhood.neighbors_
        key = (p_pc_in.pts_.data_ptr(), p_pc_out.pts_.data_ptr(), nb32.data_ptr())
        if cache is not None and cache[0] == key:
            geom = cache[1]
        else:
            geom = ops.ConvGeometry.build(pc_in.pts_, pc_out.pts_, pc_in.local_frames_, pc_out.local_frames_,
                                          nb32, p_neighborhood.start_ids_,
                                          symmetric=bool(getattr(p_neighborhood, "symmetric_", False)) and
                                          p_pc_in is p_pc_out)
            geom.edge_info = getattr(p_neighborhood, "edge_info_", None)
            geom.bounded = geom.edge_info is not None
            if geom.symmetric:
                geom.sources = getattr(p_neighborhood, "sources_i32_", None)
            geom.source_major_fn = getattr(p_neighborhood, "source_major", None)
            try:
                p_neighborhood._se3_geom_plain = (key, geom)
            except AttributeError:
                pass
        axes9 = torch.cat([self.proj_axes_, self.proj_axes_.new_zeros((6, self.num_basis_))], dim=0)
        return _conv_any_num_basis(p_in_features, axes9, self.proj_biases_, self.conv_weights_, geom,
                                   self.norm_neigh_dist_, self.norm_num_neighs_)


class PNEConvLayerFactory(IConvLayerFactory):
    """``layers/PNEConvLayer.py:232-274``."""

    def __init__(self, p_dims, p_num_basis, p_pne_type, p_aggregation="add"):
        super().__init__(p_dims)
        self.num_basis_ = p_num_basis
        self.pne_type_ = p_pne_type
        self.aggregation_ = p_aggregation

    def update_parameters(self, **kwargs):
        if "num_basis" in kwargs:
            self.num_basis_ = kwargs["num_basis"]

    def __create_conv_layer_imp__(self, p_in_features, p_out_features):
        return PNEConvLayer(self.dims_, p_in_features, p_out_features, self.num_basis_, self.pne_type_, self.aggregation_)


_KP_RES = {"single": "kp_gauss", "double": "kp_gauss_double"}  # p_kp_res -> the kernel-point set (and sigma) of that PNE type


class MultiHeadAttLayer(IConvLayer):
    """The reference's multi-head attention over the basis functions (``layers/MultiHeadAttLayer.py:11-150``):

        phi = kp_gauss(rho (x_p - y_s)) @ proj_axes_ + proj_biases_                      per edge, [E,K]
        [q v | key] = linear_kqv_(f)                                                      [N,2V] and [N,V], V = C_in
        T[s,c,k] = sum_{(s,p) in E} phi_k [q v][p,c]                                      FeatBasisProj, [N,2V,K]
        att[s,k,h] = softmax_k sum_{i in head h} (Tq[s,i,k] + pe_[k,i]) key[s,i]          ops.BasisAttention, one HIP pass
        out[s] = nu * w_out_(sum_k Tv[s,:,k] att[s,k,h(:)])

    Parameters and buffers by the reference's names and shapes (``kernel_pts_ [13|55,3]``, ``proj_axes_ [J,K]``, ``proj_biases_ [K]``,
    ``linear_kqv_``, ``w_out_``, ``pe_ [1,K,V]``) and its init bounds; the kernel points are rotated once with a uniformly drawn
    rotation.  As in the reference there is no ``1/sqrt(D)`` and the bias of ``w_out_`` is scaled by ``nu`` too (DESIGN.md "Quirks").
    ``p_num_basis`` is one of FeatBasisProj's; input and output cloud are one object; capacity-bounded neighbourhoods are refused.

    ``p_fused=True`` (the attribute ``fused_``; no parameter or buffer, so the state dict is the reference's either way) runs
    ``PneEmbed -> linear_kqv_ -> ops.FusedBasisAttention -> w_out_``: the same function edge-wise, without ``T``."""

    def __init__(self, p_dims, p_in_features, p_out_features, p_num_basis, p_kp_res, p_num_heads, p_fused=False):
        super().__init__(p_dims, p_in_features, p_out_features)
        self.fused_ = bool(p_fused)
        if p_dims != 3:
            raise NotImplementedError(f"{type(self).__name__} on the HIP library: 3-D points")
        if p_kp_res not in _KP_RES:
            raise ValueError(f"unknown kernel-point resolution {p_kp_res!r}: expected 'single' or 'double'")
        if p_num_heads < 1 or p_in_features % p_num_heads != 0:
            raise ValueError(f"{p_num_heads} heads do not divide the {p_in_features} input features")
        if p_num_basis not in _FEAT_BASIS_K:
            raise ValueError(f"{type(self).__name__} aggregates through FeatBasisProj, which takes a number of basis functions in "
                             f"{set(_FEAT_BASIS_K)}, not {p_num_basis}")
        self.num_basis_ = p_num_basis
        self.kp_res_ = p_kp_res
        self.num_heads_ = p_num_heads
        self.value_size_ = p_in_features
        self.kp_sigma_ = _KP_SETS[p_kp_res == "double"][1]["gauss"]
        kp = torch.from_numpy(kernel_points(_KP_RES[p_kp_res])) @ _random_rotation()
        self.register_buffer("kernel_pts_", kp.to(torch.float32))
        bound = math.sqrt(1.0 / kp.shape[0])
        self.proj_axes_ = torch.nn.Parameter(torch.empty(kp.shape[0], p_num_basis).uniform_(-bound, bound))
        self.proj_biases_ = torch.nn.Parameter(torch.zeros((p_num_basis,), dtype=torch.float32))
        self.linear_kqv_ = torch.nn.Linear(p_in_features, 3 * self.value_size_)
        self.w_out_ = torch.nn.Linear(self.value_size_, p_out_features)
        bound = math.sqrt(1.0 / self.value_size_)
        self.pe_ = torch.nn.Parameter(torch.empty(1, p_num_basis, self.value_size_).uniform_(-bound, bound))

    def _attend(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        """``(w_out_(attention), T)``: steps 1 to 5, before the scaling."""
        if p_pc_in is not p_pc_out:
            raise AssertionError(f"{type(self).__name__}: the input and the output cloud must be the same object, as in the reference")
        if getattr(p_neighborhood, "edge_info_", None) is not None:
            raise NotImplementedError("a capacity-bounded neighbourhood (rows past the edge count are unset) cannot feed "
                                      "the materialised path: build the neighbourhood without p_capacity")
        nb32 = getattr(p_neighborhood, "neighbors_i32_", None)
        if nb32 is None:
            nb32 = p_neighborhood.neighbors_
        v = self.value_size_
        phi = ops.PneEmbed.apply(p_pc_in.pts_, p_pc_out.pts_, nb32, self.proj_axes_, self.proj_biases_, self.norm_neigh_dist_,
                                 "kp_gauss", self.kernel_pts_, self.kp_sigma_)
        x = self.linear_kqv_(p_in_features)
        t = ops.FeatBasisProj.apply(phi, x[:, :2 * v], nb32, p_neighborhood.start_ids_)
        agg = ops.BasisAttention.apply(t, x[:, 2 * v:], self.pe_, self.num_heads_)
        return self.w_out_(agg), t

    def _attend_fused(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        """``(w_out_(attention), phi, x, nb32)`` of the edge-wise operator: no ``T``."""
        if p_pc_in is not p_pc_out:
            raise AssertionError(f"{type(self).__name__}: the input and the output cloud must be the same object, as in the reference")
        if getattr(p_neighborhood, "edge_info_", None) is not None:
            raise NotImplementedError("a capacity-bounded neighbourhood (rows past the edge count are unset) cannot feed "
                                      "the fused attention (p_fused=True): build the neighbourhood without p_capacity")
        nb32 = getattr(p_neighborhood, "neighbors_i32_", None)
        if nb32 is None:
            nb32 = p_neighborhood.neighbors_
        phi = ops.PneEmbed.apply(p_pc_in.pts_, p_pc_out.pts_, nb32, self.proj_axes_, self.proj_biases_, self.norm_neigh_dist_,
                                 "kp_gauss", self.kernel_pts_, self.kp_sigma_)
        x = self.linear_kqv_(p_in_features)
        agg = ops.FusedBasisAttention.apply(phi, x, self.pe_, nb32, p_neighborhood.start_ids_, self.num_heads_, p_neighborhood)
        return self.w_out_(agg), phi, x, nb32

    def __compute_convolution__(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        if self.fused_:
            return self._attend_fused(p_pc_in, p_pc_out, p_in_features, p_neighborhood)[0] * self.norm_num_neighs_
        return self._attend(p_pc_in, p_pc_out, p_in_features, p_neighborhood)[0] * self.norm_num_neighs_


class LoRAttConvLayer(MultiHeadAttLayer):
    """The reference's low-rank attention convolution (``layers/LoRAttConvLayer.py:11-163``): ``MultiHeadAttLayer`` plus an ordinary
    continuous convolution on the value half of the same aggregate, ``sum_{k,i} Tv[s,i,k] conv_weights_[k,i,o]``, both scaled by
    ``nu``.  ``conv_weights_ [K,V,C_out]`` as in the reference; the product reads ``Tv`` as a view of ``T``.

    ``p_fused=True``: the attention goes through ``ops.FusedBasisAttention``; the dense product keeps ``FeatBasisProj``, but over the
    ``V`` value columns only (``x[:, :V]``): ``Tv [N,V,K]``, half of the unfused ``T`` and none of its query half."""

    def __init__(self, p_dims, p_in_features, p_out_features, p_num_basis, p_kp_res, p_num_heads, p_fused=False):
        super().__init__(p_dims, p_in_features, p_out_features, p_num_basis, p_kp_res, p_num_heads, p_fused)
        bound = math.sqrt(1.0 / (self.value_size_ * p_num_basis))
        self.conv_weights_ = torch.nn.Parameter(torch.empty(p_num_basis, self.value_size_, p_out_features).uniform_(-bound, bound))

    def __compute_convolution__(self, p_pc_in, p_pc_out, p_in_features, p_neighborhood):
        v, k = self.value_size_, self.num_basis_
        w = self.conv_weights_.permute(1, 0, 2).reshape(v * k, self.feat_output_size_)
        if self.fused_:
            att, phi, x, nb32 = self._attend_fused(p_pc_in, p_pc_out, p_in_features, p_neighborhood)
            tv = ops.FeatBasisProj.apply(phi, x[:, :v], nb32, p_neighborhood.start_ids_)
            return (att + torch.matmul(tv.reshape(tv.shape[0], v * k), w)) * self.norm_num_neighs_
        att, t = self._attend(p_pc_in, p_pc_out, p_in_features, p_neighborhood)
        conv = torch.matmul(t[:, :v, :].reshape(t.shape[0], v * k), w)
        return (att + conv) * self.norm_num_neighs_


class MultiHeadAttLayerFactory(IConvLayerFactory):
    """``layers/MultiHeadAttLayer.py:153-202``."""

    _layer = MultiHeadAttLayer

    def __init__(self, p_dims, p_num_basis, p_kp_res, p_num_heads, p_fused=False):
        super().__init__(p_dims)
        self.num_basis_ = p_num_basis
        self.kp_res_ = p_kp_res
        self.num_heads_ = p_num_heads
        self.fused_ = bool(p_fused)   # handed to the layers: the edge-wise attention without T

    def update_parameters(self, **kwargs):
        # an `elif` chain, as in the reference: only the first key present is applied (DESIGN.md "Quirks")
        if "num_basis" in kwargs:
            self.num_basis_ = kwargs["num_basis"]
        elif "kp_res" in kwargs:
            self.kp_res_ = kwargs["kp_res"]
        elif "num_heads" in kwargs:
            self.num_heads_ = kwargs["num_heads"]

    def __create_conv_layer_imp__(self, p_in_features, p_out_features):
        return self._layer(self.dims_, p_in_features, p_out_features, self.num_basis_, self.kp_res_, self.num_heads_, self.fused_)


class LoRAttConvLayerFactory(MultiHeadAttLayerFactory):
    """``layers/LoRAttConvLayer.py:166-215``."""

    _layer = LoRAttConvLayer


class PNEConvLayerRotEquivFactory(IConvLayerFactory):
    def __init__(self, p_dims, p_num_basis, p_pne_type, p_rel_rot="6D"):
        super().__init__(p_dims)
        self.num_basis_ = p_num_basis
        self.pne_type_ = p_pne_type
        self.rel_rot_ = p_rel_rot

    def update_parameters(self, **kwargs):
        if "num_basis" in kwargs:
            self.num_basis_ = kwargs["num_basis"]

    def __create_conv_layer_imp__(self, p_in_features, p_out_features):
        PNEConvLayerRotEquiv.rel_rot_type = self.rel_rot_
        return PNEConvLayerRotEquiv(self.dims_, p_in_features, p_out_features, self.num_basis_, self.pne_type_)
