"""Tensor-level wrappers over the C ABI (include/mdno.h).  PyTorch is used for device memory and
streams only; every computation below is a libmdno HIP kernel.  All tensors must be CUDA(HIP)
tensors — there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._args import INT_MAX, check_dims, device_tensor, form_code, int_list, integer, operand, real, to_list
from ._lib import AGGR, KernelNNParams, MdnoError, check, f32, ptr, raise_on_status, stream_ptr


@dataclass
class CSRGraph:
    """Destination-sorted CSR (see mdno.h): row r lists the sources of its in-edges."""
    row_ptr: torch.Tensor            # i32 [R+1]
    src: torch.Tensor                # i32 [cap]
    dst: torch.Tensor                # i32 [cap]
    num_edges: torch.Tensor          # i32 [1] (device)
    edge_cap: int
    perm: Optional[torch.Tensor] = None   # i32 [E]: CSR position p holds input edge perm[p]
    status: Optional[torch.Tensor] = None
    n_edges: Optional[int] = None         # the edge count when the host knows it (COO input): no device read

    def edge_count(self) -> int:
        return self.n_edges if self.n_edges is not None else int(self.num_edges.item())

    def to_edge_index(self) -> torch.Tensor:
        """Reference-order COO `[rows; cols]` (graph_kernel.py:368) — valid for radius graphs, whose
        contact map is symmetric, so (dst, src) read in CSR order IS the row-major COO."""
        e = self.edge_count()
        return torch.stack([self.dst[:e], self.src[:e]]).to(torch.long)


def _empty_csr(R: int, cap: int, dev) -> CSRGraph:
    """The buffers a radius graph of R rows and at most `cap` edges is built into (count and status zeroed)."""
    i32 = dict(dtype=torch.int32, device=dev)
    return CSRGraph(torch.empty(R + 1, **i32), torch.empty(cap, **i32), torch.empty(cap, **i32), torch.zeros(1, **i32),
                    cap, None, torch.zeros(1, **i32))


def radius_graph(pos: torch.Tensor, n_atoms: int, cutoff: float = 8.0, edge_cap: Optional[int] = None,
                 cell_list: bool = True) -> CSRGraph:
    """pos f32 [M*N,3] (or [M,N,3]) -> CSRGraph.  Replaces graph_kernel.py:363-368.  Members of >= 8,192 atoms go
    through a cell list (`cell_list=False`: the N^2 pair tests; the same graph, bit for bit)."""
    lib = _lib.load()
    pos = f32(pos).reshape(-1, 3)
    R = pos.shape[0]
    if R % n_atoms:
        raise MdnoError(f"{R} rows is not a multiple of n_atoms={n_atoms}")
    M = R // n_atoms
    cap = int(edge_cap) if edge_cap is not None else M * n_atoms * n_atoms
    cap = max(cap, R)
    dev = pos.device
    g = _empty_csr(R, cap, dev)
    nbytes = lib.mdno_radius_graph_workspace_bytes(M, n_atoms) if cell_list else 0      # > 0: large members, cell list
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check(lib.mdno_radius_graph_csr_ws(ptr(pos), M, n_atoms, float(cutoff), ptr(g.row_ptr), ptr(g.src), ptr(g.dst), cap,
                                       ptr(g.num_edges), ptr(g.status), ptr(ws), nbytes, stream_ptr(dev)),
          "mdno_radius_graph_csr_ws")
    return g


def check_box(box, cutoff: float, what: str = "box"):
    """A periodic box (include/mdno_pbc.h) as three Python floats, or None for `box` None or all zero (no periodic
    axis: the open path).  Three finite lengths >= 0 (0 = open axis), every periodic one >= 2 * cutoff; anything else
    raises MdnoError — on the host, before any device work."""
    if box is None:
        return None
    box = to_list(box)
    try:
        vals = [float(v) for v in (box if hasattr(box, "__len__") else list(box))]
    except (TypeError, ValueError):
        raise MdnoError(f"{what}={box!r}: expected three lengths (Lx, Ly, Lz)") from None
    if len(vals) != 3:
        raise MdnoError(f"{what} has {len(vals)} entries, expected (Lx, Ly, Lz)")
    cutoff = real(cutoff, "cutoff", positive=False)
    for a, L in enumerate(vals):
        real(L, f"{what}[{a}] (a length, or 0 for an open axis)", positive=False)
        if L != 0.0 and not L >= 2.0 * cutoff:
            raise MdnoError(f"{what}[{a}] = {L} < 2 * cutoff = {2.0 * cutoff}: a pair would have more than one image "
                            f"inside the cutoff")
    return tuple(vals) if any(v > 0.0 for v in vals) else None


def box_arg(box):
    """(Lx, Ly, Lz) as the host `const double*` the C ABI takes (keep the returned array alive across the call)."""
    return (C.c_double * 3)(*box)


def radius_graph_pbc(pos: torch.Tensor, n_atoms: int, cutoff: float, box, edge_cap: Optional[int] = None,
                     with_attr: bool = True):
    """Periodic radius graph (include/mdno_pbc.h): pos f32 [M*N,3] (or [M,N,3]), box = (Lx, Ly, Lz) with 0 for an open
    axis -> (CSRGraph, edge_attr f32 [edge_cap, 6] or None).  Row p of edge_attr is [image of pos[src[p]] next to the
    destination, pos[dst[p]]]; rows from the edge count on are not written.  Brute force at every size."""
    vals = check_box(box, cutoff)
    if vals is None:
        vals = (0.0, 0.0, 0.0)      # no periodic axis: the open graph, with its attributes
    pos = device_tensor(pos, "pos", None).reshape(-1, 3)
    lib = _lib.load()
    R = pos.shape[0]
    if n_atoms <= 0 or R == 0 or R % n_atoms:
        raise MdnoError(f"{R} rows is not a positive multiple of n_atoms={n_atoms}")
    M = R // n_atoms
    cap = int(edge_cap) if edge_cap is not None else M * n_atoms * n_atoms
    cap = max(cap, R)
    dev = pos.device
    g = _empty_csr(R, cap, dev)
    attr = torch.empty((cap, 6), dtype=torch.float32, device=dev) if with_attr else None
    b = box_arg(vals)
    check(lib.mdno_radius_graph_pbc(ptr(pos), M, n_atoms, float(cutoff), b, ptr(g.row_ptr), ptr(g.src), ptr(g.dst), ptr(attr),
                                    cap, ptr(g.num_edges), ptr(g.status), stream_ptr(dev)), "mdno_radius_graph_pbc")
    return g, attr


def coo_to_csr(edge_index: torch.Tensor, num_nodes: int, validate: bool = True,
               status: Optional[torch.Tensor] = None) -> CSRGraph:
    """edge_index i64 [2,E] (row 0 = source, row 1 = target) -> CSRGraph with `perm`.  A node id
    outside [0, num_nodes) raises (as the reference's gather / scatter do); `validate=False` defers
    that check: the bit stays in `graph.status` (`status` if given: a device word the kernels OR into)
    for the caller to read after its own work — no host synchronisation here."""
    lib = _lib.load()
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise MdnoError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
    ei = edge_index.to(torch.long).contiguous()
    E = ei.shape[1]
    dev = ei.device
    row_ptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    cap = max(E, 1)
    src = torch.empty(cap, dtype=torch.int32, device=dev)
    dst = torch.empty(cap, dtype=torch.int32, device=dev)
    perm = torch.empty(cap, dtype=torch.int32, device=dev)
    nbytes = lib.mdno_coo_to_csr_workspace_bytes(E, num_nodes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    ne = torch.empty(1, dtype=torch.int32, device=dev)       # written by the sort itself (no fill launch)
    check(lib.mdno_coo_to_csr(ptr(ei), E, num_nodes, ptr(row_ptr), ptr(src), ptr(dst), ptr(perm), ptr(ne), ptr(status),
                              ptr(ws), nbytes, stream_ptr(dev)), "mdno_coo_to_csr")
    if validate:
        raise_on_status(status.item(), "coo_to_csr")
    return CSRGraph(row_ptr, src, dst, ne, cap, perm, status, n_edges=E)


def edge_mlp(weights, ker_in: int, ker_width: int, out_dim: int, graph: CSRGraph,
             edge_pos: Optional[torch.Tensor] = None, edge_attr: Optional[torch.Tensor] = None,
             gemm_mode: str = "split_bf16") -> torch.Tensor:
    """W_e f32 [cap, out_dim] in CSR edge order.  `weights` = (w0,b0,w1,b1,w2,b2) torch Linear
    layout.  Attributes from `edge_pos` [R,3] + CSR, or `edge_attr` [E,ker_in] (+ graph.perm)."""
    lib = _lib.load()
    w = [f32(t) for t in weights]
    dev = w[0].device
    cap = graph.edge_cap
    w_e = torch.empty((cap, out_dim), dtype=torch.float32, device=dev)
    mode = _lib.GEMM_MODES[gemm_mode]
    nbytes = lib.mdno_edge_mlp_workspace_bytes(ker_width, out_dim, cap, mode)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ea = f32(edge_attr) if edge_attr is not None else None
    ep = f32(edge_pos).reshape(-1, 3) if edge_pos is not None else None
    check(lib.mdno_edge_mlp_fwd(ptr(ep), ptr(graph.src), ptr(graph.dst), ptr(ea),
                                ptr(graph.perm) if ea is not None else None, ptr(graph.num_edges), cap,
                                ker_in, ker_width, out_dim, mode, *[ptr(t) for t in w], ptr(w_e), ptr(ws), nbytes,
                                stream_ptr(dev)), "mdno_edge_mlp_fwd")
    return w_e


def nnconv(x: torch.Tensor, graph: CSRGraph, w_e: torch.Tensor, root: Optional[torch.Tensor],
           bias: Optional[torch.Tensor], aggr: str = "mean", relu: bool = False,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    if aggr not in AGGR:
        raise MdnoError(f"aggr={aggr!r} is not implemented by the HIP path (add, mean)")
    x = f32(x)
    R, cin = x.shape
    cout = w_e.shape[1] // cin
    y = out if out is not None else torch.empty((R, cout), dtype=torch.float32, device=x.device)
    root_c = f32(root) if root is not None else None
    bias_c = f32(bias) if bias is not None else None
    if w_e.shape[0] == 0:       # no edges: every row is x.root + bias and W_e is never read, but must not be null
        w_e = torch.empty((1, cin * cout), dtype=torch.float32, device=x.device)
    check(lib.mdno_nnconv_fwd(ptr(x), ptr(graph.row_ptr), ptr(graph.src), R, ptr(w_e), ptr(root_c), ptr(bias_c),
                              cin, cout, AGGR[aggr], int(relu), ptr(y), stream_ptr(x.device)), "mdno_nnconv_fwd")
    return y


class ParamPack:
    """Owns contiguous fp32 device copies (or views) of a KernelNN state_dict and the C struct
    pointing at them.  Keep it alive while kernels that use it are in flight."""

    KEYS = {
        "lstm_w_ih": "lstm.weight_ih_l0", "lstm_w_hh": "lstm.weight_hh_l0",
        "lstm_b_ih": "lstm.bias_ih_l0", "lstm_b_hh": "lstm.bias_hh_l0",
        "lstm_fc_w": "lstm_fc.weight", "lstm_fc_b": "lstm_fc.bias", "emb_w": "emb.weight",
        "fc1_w": "fc1.weight", "fc1_b": "fc1.bias",
        "k_w0": "conv1.net.layers.0.weight", "k_b0": "conv1.net.layers.0.bias",
        "k_w1": "conv1.net.layers.2.weight", "k_b1": "conv1.net.layers.2.bias",
        "k_w2": "conv1.net.layers.4.weight", "k_b2": "conv1.net.layers.4.bias",
        "k2_w0": "conv2.net.layers.0.weight", "k2_b0": "conv2.net.layers.0.bias",
        "k2_w1": "conv2.net.layers.2.weight", "k2_b1": "conv2.net.layers.2.bias",
        "k2_w2": "conv2.net.layers.4.weight", "k2_b2": "conv2.net.layers.4.bias",
        "conv1_root": "conv1.root", "conv1_bias": "conv1.bias",
        "conv2_root": "conv2.root", "conv2_bias": "conv2.bias",
        "fc2_w": "fc2.weight", "fc2_b": "fc2.bias",
    }

    def __init__(self, state_dict, depth: int, device, gemm_mode: str = "split_bf16",
                 conv_mode: str = "materialized"):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        self._check_dims(sd)
        self.tensors = {}
        p = KernelNNParams()
        for field, key in self.KEYS.items():
            if key not in sd:
                # optional groups: conv2's own kernel (shared otherwise), and — notebook-era model
                # (bba_analysis.ipynb:123-128) — the LSTM front-end and the whole conv2 block
                if field.startswith(("k2_", "lstm_", "conv2_")):
                    setattr(p, field, None)
                    continue
                raise MdnoError(f"state_dict lacks {key!r}")
            t = sd[key].detach().to(device=device, dtype=torch.float32).contiguous()
            self.tensors[field] = t
            if t.numel() == 0:          # embedding_dim 0: an empty table has no storage; the kernels never read it
                t = self.tensors.setdefault("_empty", torch.zeros(4, dtype=torch.float32, device=device))
            setattr(p, field, t.data_ptr())
        # the reference shares ONE edge-MLP between conv1 and conv2 (graph_kernel.py:271-273):
        # tied storage or equal values -> evaluate once
        shared = all(
            ("k2_" + n) not in self.tensors
            or self.tensors["k2_" + n].data_ptr() == self.tensors["k_" + n].data_ptr()
            or torch.equal(self.tensors["k2_" + n], self.tensors["k_" + n])
            for n in ("w0", "b0", "w1", "b1", "w2", "b2"))
        if shared:
            for n in ("w0", "b0", "w1", "b1", "w2", "b2"):
                setattr(p, "k2_" + n, None)
        self.shared_kernel = shared
        width = self.tensors["fc1_w"].shape[0]
        p.width = width
        p.ker_width = self.tensors["k_w0"].shape[0]
        p.depth = int(depth)
        p.ker_in = self.tensors["k_w0"].shape[1]
        p.in_width = self.tensors["fc1_w"].shape[1]
        p.out_width = self.tensors["fc2_w"].shape[0]
        p.num_embeddings, p.embedding_dim = self.tensors["emb_w"].shape
        p.x_position_dim = self.tensors["lstm_w_ih"].shape[1] if "lstm_w_ih" in self.tensors else 3
        if ("lstm_w_ih" in self.tensors) != ("lstm_fc_w" in self.tensors) or \
                ("conv2_root" in self.tensors) != ("conv2_bias" in self.tensors):
            raise MdnoError("state_dict has a partial lstm/conv2 parameter group")
        p.gemm_mode = _lib.GEMM_MODES[gemm_mode]
        self.gemm_mode = gemm_mode
        p.conv_mode = _lib.CONV_MODES[conv_mode]
        self.conv_mode = conv_mode
        if self.tensors["k_w2"].shape[0] != width * width:
            raise MdnoError("edge-MLP output size != width**2")
        self.struct = p
        self.device = torch.device(device)

    @staticmethod
    def _check_dims(sd) -> None:
        """The limits of the kernels (csrc/node_ops.hip, csrc/edge_mlp.hip), checked on the host before anything is
        copied to the device."""
        if "emb.weight" in sd and "fc1.weight" in sd:
            emb = sd["emb.weight"].shape[1]
            if emb > 16:
                raise MdnoError(f"embedding_dim={emb} (0..16)")
            if sd["fc1.weight"].shape[1] != emb + 3:
                raise MdnoError(f"in_width={sd['fc1.weight'].shape[1]} must equal embedding_dim + 3 = {emb + 3} "
                                "(graph_kernel.py:296)")
        w0 = sd.get("conv1.net.layers.0.weight")
        if w0 is not None and not 1 <= w0.shape[1] <= 8:
            raise MdnoError(f"ker_in={w0.shape[1]} (1..8)")

    @property
    def ref(self):
        return C.byref(self.struct)


def node_prologue(pack: ParamPack, frames: torch.Tensor, x_aminoacid: torch.Tensor,
                  status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames f32 [W,M,N,3] -> x0 f32 [M*N,width]: LSTM over the window, lstm_fc, Embedding, concat, fc1,
    ReLU (graph_kernel.py:279-298).  Raises on an amino-acid id outside [0, num_embeddings) — unless the
    caller passes its own `status` word (int32 [1] on the device): the bit is then left there for it to
    read later and this call does not synchronise."""
    lib = _lib.load()
    frames = f32(frames)
    if frames.dim() == 3:
        frames = frames.unsqueeze(1)
    W, M, N, _ = frames.shape
    dev = frames.device
    aa = x_aminoacid.to(device=dev, dtype=torch.long).contiguous()
    if aa.numel() not in (N, M * N):
        raise MdnoError(f"x_aminoacid has {aa.numel()} entries, expected {N} or {M * N}")
    x0 = out if out is not None else torch.empty((M * N, pack.struct.width), dtype=torch.float32, device=dev)
    if tuple(x0.shape) != (M * N, pack.struct.width) or x0.dtype != torch.float32:
        raise MdnoError(f"node_prologue: out must be f32 {(M * N, pack.struct.width)}")
    deferred = status is not None
    if not deferred:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.mdno_node_prologue_fwd(pack.ref, ptr(frames), M, W, N, ptr(aa), int(aa.numel() == M * N and M > 1),
                                     ptr(x0), ptr(status), stream_ptr(dev)), "mdno_node_prologue_fwd")
    if not deferred:
        raise_on_status(status.item(), "node_prologue")
    return x0


FALLBACK_KEYS = ("conv_k1_workgroups_rerun_bf16", "conv_destinations_unscaled", "edge_mlp_products_bf16")


def kernelnn_forward(pack: ParamPack, frames: torch.Tensor, x_aminoacid: torch.Tensor, graph: CSRGraph,
                     edge_pos: Optional[torch.Tensor] = None, edge_attr: Optional[torch.Tensor] = None,
                     return_latent: bool = False, workspace: Optional[torch.Tensor] = None,
                     check_status: bool = True, fallback_counts: Optional[dict] = None
                     ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """frames f32 [W,M,N,3] (time-major) -> out [M*N,out_width] (+ latent [M*N,width]).
    `fallback_counts`: a dict that receives which path gemm_mode "split_f16" took in this forward (FALLBACK_KEYS:
    all zero = every product on two fp16 planes; include/mdno.h mdno_kernelnn_fallback_counts) — reading it
    synchronises the stream.
    The device status word (bad amino-acid id, edge overflow, bad edge index) is read back and
    raised after the call — the reference's nn.Embedding raises IndexError at that point; pass
    `check_status=False` to keep the call asynchronous and read `graph.status` yourself."""
    lib = _lib.load()
    frames = f32(frames)
    if frames.dim() == 3:
        frames = frames.unsqueeze(1)
    W, M, N, _ = frames.shape
    dev = frames.device
    aa = x_aminoacid.to(device=dev, dtype=torch.long).contiguous()
    if aa.numel() not in (N, M * N):
        raise MdnoError(f"x_aminoacid has {aa.numel()} entries, expected {N} or {M * N}")
    aa_pm = int(aa.numel() == M * N and M > 1)
    p = pack.struct
    out = torch.empty((M * N, p.out_width), dtype=torch.float32, device=dev)
    latent = torch.empty((M * N, p.width), dtype=torch.float32, device=dev) if return_latent else None
    nbytes = lib.mdno_kernelnn_workspace_bytes(pack.ref, M, N, graph.edge_cap)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if graph.status is None:
        graph.status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = graph.status
    ea = f32(edge_attr) if edge_attr is not None else None
    ep = f32(edge_pos).reshape(-1, 3) if edge_pos is not None else None
    if ea is None and ep is None:
        raise MdnoError("kernelnn_forward needs edge_pos (a library-built radius graph) or edge_attr")
    check(lib.mdno_kernelnn_fwd(pack.ref, ptr(frames), M, W, N, ptr(aa), aa_pm, ptr(graph.row_ptr), ptr(graph.src),
                                ptr(graph.dst), ptr(graph.num_edges), graph.edge_cap, ptr(ep),
                                ptr(ea),
                                ptr(graph.perm) if ea is not None else None, ptr(out), ptr(latent), ptr(workspace),
                                workspace.numel(), ptr(status), stream_ptr(dev)), "mdno_kernelnn_fwd")
    if fallback_counts is not None:
        cnt = (C.c_int64 * 4)()
        check(lib.mdno_kernelnn_fallback_counts(pack.ref, M, N, graph.edge_cap, int(ep is not None and ea is None and graph.dst is not None),
                                                ptr(workspace), cnt, stream_ptr(dev)), "mdno_kernelnn_fallback_counts")
        fallback_counts.update({k: int(cnt[i]) for i, k in enumerate(FALLBACK_KEYS)})
    if check_status:
        raise_on_status(status.item(), "kernelnn_forward")
    return out, latent


class AdamTensor(C.Structure):
    """include/mdno.h mdno_adam_tensor"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64)]


def adam_step(params, grads, exp_avgs, exp_avg_sqs, lr: float, beta1: float, beta2: float, eps: float,
              weight_decay: float, step: int) -> None:
    """torch.optim.Adam's update (L2 weight decay, no amsgrad) of all the given fp32 tensors in ONE launch
    (include/mdno.h mdno_adam_step), in place, on the current stream."""
    n = len(params)
    if n == 0:
        return
    arr = (AdamTensor * n)()
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        if not (p.dtype == g.dtype == m.dtype == v.dtype == torch.float32):
            raise MdnoError("adam_step: fp32 tensors only")
        if not (p.numel() == g.numel() == m.numel() == v.numel()):
            raise MdnoError("adam_step: parameter, gradient and moments must have the same number of elements")
        arr[i] = AdamTensor(ptr(p), ptr(g), ptr(m), ptr(v), p.numel())
    check(_lib.load().mdno_adam_step(n, arr, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                     stream_ptr(params[0].device)), "mdno_adam_step")


class FlatTensor(C.Structure):
    """include/mdno.h mdno_flat_tensor"""
    _fields_ = [("data", C.c_void_p), ("numel", C.c_int64), ("offset", C.c_int64)]


def _flat_table(tensors, flat: Optional[torch.Tensor], offsets, what: str):
    if len(tensors) != len(offsets):
        raise MdnoError(f"{what}: {len(tensors)} tensors but {len(offsets)} offsets")
    if flat is not None and flat.dtype != torch.float32:
        raise MdnoError(f"{what}: the flat buffer must be fp32")
    arr = (FlatTensor * max(len(tensors), 1))()
    for i, (t, off) in enumerate(zip(tensors, offsets)):
        if isinstance(t, int):                 # (pack only) a slot of this many elements without data: zero-filled
            data, n = None, t
        else:
            if t.dtype != torch.float32:
                raise MdnoError(f"{what}: fp32 tensors only (tensor {i} is {t.dtype})")
            data, n = ptr(t), t.numel()
        # the library cannot see the flat buffer's size: the slot must lie inside it
        if flat is not None and int(off) >= 0 and n >= 0 and int(off) + n > flat.numel():
            raise MdnoError(f"{what}: slot {i} [{int(off)}, {int(off) + n}) lies outside the flat buffer of {flat.numel()}")
        arr[i] = FlatTensor(data, n, int(off))
    return arr


def pack_tensors(tensors, flat: torch.Tensor, offsets) -> torch.Tensor:
    """flat[offsets[i] : offsets[i] + numel_i] = tensors[i] for every fp32 tensor of the list, in ONE launch
    (include/mdno.h mdno_pack_tensors), on the current stream.  An entry given as an int n instead of a tensor
    zero-fills a slot of n elements.  Returns flat."""
    arr = _flat_table(tensors, flat, offsets, "pack_tensors")
    check(_lib.load().mdno_pack_tensors(len(tensors), arr, ptr(flat), stream_ptr(flat.device if flat is not None else None)),
          "mdno_pack_tensors")
    return flat


def unpack_tensors(flat: torch.Tensor, tensors, offsets) -> None:
    """tensors[i] (in place) = flat[offsets[i] : offsets[i] + numel_i], in ONE launch (include/mdno.h
    mdno_unpack_tensors), on the current stream."""
    arr = _flat_table(tensors, flat, offsets, "unpack_tensors")
    check(_lib.load().mdno_unpack_tensors(len(tensors), arr, ptr(flat), stream_ptr(flat.device if flat is not None else None)),
          "mdno_unpack_tensors")


# ------------------------------------------------------------------------------------------------
# Training ops (include/mdno.h "Training ops"): thin wrappers, torch only allocates the outputs.
def _ws(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _aligned16(*tensors) -> bool:
    """What the split-plane entry points ask of their operands (a contiguous view may start anywhere in its buffer)."""
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def linear(a: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], relu: bool = False,
           gemm_mode: str = "f32") -> torch.Tensor:
    """act(a . w^T + b): a [rows,k], w [n,k] (torch Linear layout).  gemm_mode "split_bf16" runs the
    product on the bf16 matrix pipe with the exact 3-way split (fp32-level error), "split_f16" on two fp16
    planes per operand with every row scaled by its own power of two (3 products instead of 6, fp32-level
    error), where the shape tiles (k % 32 == 0, n % 128 == 0) and a, w are 16-byte aligned; other shapes, misaligned
    views and "f32" use the fp32 kernels."""
    lib = _lib.load()
    a, w = f32(a), f32(w)
    rows, k = a.shape
    n = w.shape[0]
    c = torch.empty((rows, n), dtype=torch.float32, device=a.device)
    if rows == 0:               # (an edge network over a graph without edges)
        return c
    bb = f32(b) if b is not None else None
    tiles = k % 32 == 0 and n % 128 == 0 and rows > 0 and _aligned16(a, w)
    if gemm_mode == "split_f16" and tiles:
        ws = _ws(lib.mdno_linear_split_f16_workspace_bytes(rows, n, k), a.device)
        check(lib.mdno_linear_split_f16_fwd(ptr(a), ptr(w), ptr(bb), rows, n, k, int(relu), ptr(c), ptr(ws), ws.numel(),
                                            stream_ptr(a.device)), "mdno_linear_split_f16_fwd")
        return c
    if gemm_mode != "f32" and tiles:
        ws = _ws(lib.mdno_linear_split_workspace_bytes(rows, n, k), a.device)
        check(lib.mdno_linear_split_fwd(ptr(a), ptr(w), ptr(bb), rows, n, k, int(relu), ptr(c), ptr(ws), ws.numel(),
                                        stream_ptr(a.device)), "mdno_linear_split_fwd")
        return c
    check(lib.mdno_linear_fwd(ptr(a), ptr(w), ptr(bb), rows, n, k, int(relu), ptr(c), stream_ptr(a.device)),
          "mdno_linear_fwd")
    return c


def gemm_atb(a: torch.Tensor, b: torch.Tensor, gemm_mode: str = "f32") -> torch.Tensor:
    """a^T . b over rows: a [rows,n1], b [rows,n2] -> [n1,n2] (fixed-order partial sums).  gemm_mode "split_f16":
    on two fp16 planes per operand, columns scaled by powers of two (fp32-level error), where the shape tiles
    (n1, n2 multiples of 256) and a, b are 16-byte aligned; otherwise the fp32 kernels."""
    lib = _lib.load()
    a, b = f32(a), f32(b)
    rows, n1 = a.shape
    n2 = b.shape[1]
    c = torch.empty((n1, n2), dtype=torch.float32, device=a.device)
    if rows == 0:               # an empty sum
        return c.zero_()
    if gemm_mode == "split_f16" and lib.mdno_gemm_atb_split_f16_supported(rows, n1, n2) and _aligned16(a, b):
        ws = _ws(lib.mdno_gemm_atb_split_f16_workspace_bytes(rows, n1, n2), a.device)
        check(lib.mdno_gemm_atb_split_f16(ptr(a), ptr(b), rows, n1, n2, ptr(c), 0, ptr(ws), ws.numel(), stream_ptr(a.device)),
              "mdno_gemm_atb_split_f16")
        return c
    nb = lib.mdno_reduce_workspace_bytes(n1, n2)
    ws = _ws(nb, a.device)
    check(lib.mdno_gemm_atb(ptr(a), ptr(b), rows, n1, n2, ptr(c), 0, ptr(ws), ws.numel(), stream_ptr(a.device)),
          "mdno_gemm_atb")
    return c


def colsum(a: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a = f32(a)
    rows, n = a.shape
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    if rows == 0:               # an empty sum
        return out.zero_()
    ws = _ws(lib.mdno_reduce_workspace_bytes(n, 1), a.device)
    check(lib.mdno_colsum(ptr(a), rows, n, ptr(out), 0, ptr(ws), ws.numel(), stream_ptr(a.device)), "mdno_colsum")
    return out


def relu_bwd(g: torch.Tensor, y: torch.Tensor, row_scale: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    g, y = f32(g), f32(y)
    rows, n = g.shape
    if out is None:
        out = torch.empty_like(g)
    check(lib.mdno_relu_bwd(ptr(g), ptr(y), ptr(row_scale), rows, n, ptr(out), stream_ptr(g.device)), "mdno_relu_bwd")
    return out


def relu_bwd2(g: torch.Tensor, y: torch.Tensor, row_scale: torch.Tensor, gz: torch.Tensor, gs: torch.Tensor) -> None:
    """gz = g * (y > 0), gs = gz * row_scale[row] (both written in place)."""
    lib = _lib.load()
    g, y = f32(g), f32(y)
    rows, n = g.shape
    check(lib.mdno_relu_bwd2(ptr(g), ptr(y), ptr(row_scale), rows, n, ptr(gz), ptr(gs), stream_ptr(g.device)),
          "mdno_relu_bwd2")


def transpose(a: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a = f32(a)
    r, c = a.shape
    at = torch.empty((c, r), dtype=torch.float32, device=a.device)
    check(lib.mdno_transpose(ptr(a), r, c, ptr(at), stream_ptr(a.device)), "mdno_transpose")
    return at


def inv_degree(graph: CSRGraph, aggr: str = "mean") -> torch.Tensor:
    lib = _lib.load()
    rows = graph.row_ptr.numel() - 1
    inv = torch.empty(rows, dtype=torch.float32, device=graph.row_ptr.device)
    check(lib.mdno_inv_degree(ptr(graph.row_ptr), rows, AGGR[aggr], ptr(inv), stream_ptr(inv.device)), "mdno_inv_degree")
    return inv


def source_sorted(graph: CSRGraph, num_nodes: int, status: Optional[torch.Tensor] = None) -> CSRGraph:
    """The same edges grouped by SOURCE (include/mdno.h mdno_csr_by_source): row_ptr over sources, `src` field =
    destination of each out-edge, `perm` = the edge's position in the destination-sorted arrays (and in W_e)."""
    lib = _lib.load()
    E = graph.edge_count()
    dev = graph.row_ptr.device
    cap = max(E, 1)
    row_ptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    nbr = torch.empty(cap, dtype=torch.int32, device=dev)
    rowid = torch.empty(cap, dtype=torch.int32, device=dev)
    perm = torch.empty(cap, dtype=torch.int32, device=dev)
    nbytes = lib.mdno_coo_to_csr_workspace_bytes(E, num_nodes)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = status if status is not None else graph.status        # (ids come from a CSR that was validated when built)
    check(lib.mdno_csr_by_source(ptr(graph.src), ptr(graph.dst), E, num_nodes, ptr(row_ptr), ptr(nbr), ptr(rowid), ptr(perm),
                                 ptr(st), ptr(ws), nbytes, stream_ptr(dev)), "mdno_csr_by_source")
    return CSRGraph(row_ptr, nbr, rowid, graph.num_edges, cap, perm, st, n_edges=E)


def permute_rows(x: torch.Tensor, perm: torch.Tensor, rows: int) -> torch.Tensor:
    """out[p] = x[perm[p]] for p < rows (include/mdno.h mdno_permute_rows): per-edge rows into a graph's CSR order."""
    lib = _lib.load()
    x = f32(x)
    out = torch.empty((rows,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    width = int(x[0].numel()) if x.shape[0] else 1
    check(lib.mdno_permute_rows(ptr(x), ptr(perm), rows, width, ptr(out), stream_ptr(x.device)), "mdno_permute_rows")
    return out


def _nnconv_bwd_x(gz: torch.Tensor, gs: torch.Tensor, by_src: CSRGraph, w_e: torch.Tensor, root, bf16w: bool) -> torch.Tensor:
    """g_prev [R,64] of one conv application; `bf16w`: w_e is stored in bf16 (the entry takes no channel counts)."""
    lib = _lib.load()
    name = "mdno_nnconv_bwd_x_bf16w" if bf16w else "mdno_nnconv_bwd_x"
    g_prev = torch.empty_like(gz)
    check(getattr(lib, name)(ptr(gz), ptr(gs), ptr(by_src.row_ptr), ptr(by_src.perm), ptr(by_src.src), gz.shape[0],
                             ptr(_bf16(w_e) if bf16w else w_e), ptr(f32(root)) if root is not None else None,
                             *(() if bf16w else (64, 64)), ptr(g_prev), stream_ptr(gz.device)), name)
    return g_prev


def nnconv_bwd_x(gz: torch.Tensor, gs: torch.Tensor, by_src: CSRGraph, w_e: torch.Tensor,
                 root: Optional[torch.Tensor]) -> torch.Tensor:
    return _nnconv_bwd_x(gz, gs, by_src, w_e, root, bf16w=False)


def nnconv_bwd_root(x: torch.Tensor, gz: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x, gz [rows,64] (layers stacked along rows) -> (d_root [64,64], d_bias [64])."""
    lib = _lib.load()
    x, gz = f32(x), f32(gz)
    rows = x.shape[0]
    d_root = torch.empty((64, 64), dtype=torch.float32, device=x.device)
    d_bias = torch.empty(64, dtype=torch.float32, device=x.device)
    ws = _ws(lib.mdno_nnconv_bwd_root_workspace_bytes(rows), x.device)
    check(lib.mdno_nnconv_bwd_root(ptr(x), ptr(gz), rows, 64, 64, ptr(d_root), ptr(d_bias), 0, ptr(ws), ws.numel(),
                                   stream_ptr(x.device)), "mdno_nnconv_bwd_root")
    return d_root, d_bias


def nnconv_bwd_root_pair(x_layers: torch.Tensor, gz_layers: torch.Tensor):
    """x_layers, gz_layers [2*depth, R, 64] (conv1's applications first, then conv2's) ->
    (d_root1, d_bias1, d_root2, d_bias2): both convs' root / bias gradients from one launch, bitwise what two
    `nnconv_bwd_root` calls on the halves return."""
    lib = _lib.load()
    x, gz = f32(x_layers), f32(gz_layers)
    L, R, _ = x.shape
    assert L % 2 == 0 and gz.shape == x.shape
    rows_each = (L // 2) * R
    outs = [torch.empty(sh, dtype=torch.float32, device=x.device) for sh in ((64, 64), (64,), (64, 64), (64,))]
    ws = _ws(lib.mdno_nnconv_bwd_root_pair_workspace_bytes(rows_each), x.device)
    check(lib.mdno_nnconv_bwd_root_pair(ptr(x), ptr(gz), rows_each, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
                                        ptr(ws), ws.numel(), stream_ptr(x.device)), "mdno_nnconv_bwd_root_pair")
    return tuple(outs)


def _nnconv_bwd_we(x_layers: torch.Tensor, gs_layers: torch.Tensor, graph: CSRGraph, with_colsum: bool, bf16: bool):
    """x_layers, gs_layers [L,R,64] -> d_we [E,4096], fp32 or (`bf16`) rounded once to bf16; `with_colsum`: also its
    column sums (fp32 [4096], of the stored values) from the same pass — up to 16 conv applications (depth <= 8): the
    matrix-pipe kernel; beyond, the FMA kernel and a column-sum pass."""
    lib = _lib.load()
    L, R, _ = x_layers.shape
    e = graph.edge_count()
    dev = x_layers.device
    d_we = torch.empty((e, 4096), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    operands = (ptr(x_layers), ptr(gs_layers), ptr(graph.src), ptr(graph.dst), e, L, R * 64)
    if with_colsum and L <= 16 and e > 0:
        name = "mdno_nnconv_bwd_we_bf16_colsum" if bf16 else "mdno_nnconv_bwd_we_colsum"
        cs = torch.empty(4096, dtype=torch.float32, device=dev)
        nb = getattr(lib, name + "_workspace_bytes")()
        ws = _ws(nb, dev)
        check(getattr(lib, name)(*operands, ptr(d_we), ptr(cs), ptr(ws), nb, stream_ptr(dev)), name)
        return d_we, cs
    if bf16:
        check(lib.mdno_nnconv_bwd_we_bf16(*operands, ptr(d_we), stream_ptr(dev)), "mdno_nnconv_bwd_we_bf16")
    else:
        check(lib.mdno_nnconv_bwd_we(*operands, 64, 64, ptr(d_we), 0, stream_ptr(dev)), "mdno_nnconv_bwd_we")
    return (d_we, colsum_bf16(d_we) if bf16 else colsum(d_we)) if with_colsum else d_we


def nnconv_bwd_we(x_layers: torch.Tensor, gs_layers: torch.Tensor, graph: CSRGraph, with_colsum: bool = False):
    """d_we fp32 [E,4096] (and its column sums): see `_nnconv_bwd_we`."""
    return _nnconv_bwd_we(x_layers, gs_layers, graph, with_colsum, bf16=False)


# ------------------------------------------------------------------------------------------------
# Training ops, bf16 (include/mdno.h "Training ops, bf16"): torch only allocates; dtype torch.bfloat16
# tensors are the bf16 buffers of the C ABI.
def _bf16(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.bfloat16:
        raise MdnoError(f"expected a bfloat16 tensor, got {t.dtype}")
    return t.contiguous()


def cast_bf16(a: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a = f32(a)
    if a.numel() % 4:
        raise MdnoError("cast_bf16: element count must be a multiple of 4")
    out = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device)
    check(lib.mdno_cast_bf16(ptr(a), a.numel(), ptr(out), stream_ptr(a.device)), "mdno_cast_bf16")
    return out


def linear_smallk_bf16(a: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], relu: bool = False) -> torch.Tensor:
    """bf16(act(a . w^T + b)) for the first edge-MLP layer: a fp32 [rows,k<=8] (edge attributes), w fp32 [n,k]."""
    lib = _lib.load()
    a, w = f32(a), f32(w)
    rows, k = a.shape
    n = w.shape[0]
    if not (1 <= k <= 8 and n % 8 == 0):        # (other shapes: the fp32 kernel, then the cast)
        return cast_bf16(linear(a, w, b, relu=relu))
    c = torch.empty((rows, n), dtype=torch.bfloat16, device=a.device)
    check(lib.mdno_linear_smallk_bf16_fwd(ptr(a), ptr(w), ptr(f32(b)) if b is not None else None, rows, n, k, int(relu),
                                          ptr(c), stream_ptr(a.device)), "mdno_linear_smallk_bf16_fwd")
    return c


def linear_bf16(a: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], relu: bool = False,
                out_bf16: bool = True) -> torch.Tensor:
    """act(a . w^T + b): a bf16 [rows,k], w fp32 master [n,k] (cast per call), fp32 accumulation."""
    lib = _lib.load()
    a, w = _bf16(a), f32(w)
    rows, k = a.shape
    n = w.shape[0]
    c = torch.empty((rows, n), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a.device)
    ws = _ws(lib.mdno_linear_bf16_workspace_bytes(n, k), a.device)
    check(lib.mdno_linear_bf16_fwd(ptr(a), ptr(w), ptr(f32(b)) if b is not None else None, rows, n, k, int(relu),
                                   int(out_bf16), ptr(c), ptr(ws), ws.numel(), stream_ptr(a.device)), "mdno_linear_bf16_fwd")
    return c


def linear_bf16_relu_bwd(g: torch.Tensor, w_t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """bf16((y > 0) * (g . w_t^T)): the input gradient of a Linear + ReLU layer whose stored (bf16) output is y —
    g bf16 [rows,k], w_t fp32 [n,k] (the layer's weight, transposed), y bf16 [rows,n].  One GEMM with the mask in its
    epilogue where the shape tiles (n % 256 == 0, k % 32 == 0); otherwise the GEMM, then mdno_relu_bwd_bf16 —
    the same fp32 accumulation, mask and single rounding either way."""
    lib = _lib.load()
    g, w_t, y = _bf16(g), f32(w_t), _bf16(y)
    rows, k = g.shape
    n = w_t.shape[0]
    if not lib.mdno_linear_bf16_masked_supported(rows, n, k):
        return relu_bwd_bf16(linear_bf16(g, w_t, None, out_bf16=False), y, out_bf16=True)
    c = torch.empty((rows, n), dtype=torch.bfloat16, device=g.device)
    ws = _ws(lib.mdno_linear_bf16_workspace_bytes(n, k), g.device)
    check(lib.mdno_linear_bf16_masked(ptr(g), ptr(w_t), ptr(y), rows, n, k, ptr(c), ptr(ws), ws.numel(),
                                      stream_ptr(g.device)), "mdno_linear_bf16_masked")
    return c


def gemm_atb_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a, b = _bf16(a), _bf16(b)
    rows, n1 = a.shape
    n2 = b.shape[1]
    c = torch.empty((n1, n2), dtype=torch.float32, device=a.device)
    ws = _ws(lib.mdno_gemm_atb_bf16_workspace_bytes(n1, n2), a.device)
    check(lib.mdno_gemm_atb_bf16(ptr(a), ptr(b), rows, n1, n2, ptr(c), ptr(ws), ws.numel(), stream_ptr(a.device)),
          "mdno_gemm_atb_bf16")
    return c


def nnconv_bf16w(x: torch.Tensor, graph: CSRGraph, w_e: torch.Tensor, root, bias, aggr: str = "mean",
                 relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    x, w_e = f32(x), _bf16(w_e)
    if x.shape[1] != 64 or w_e.shape[1] != 4096:
        raise MdnoError("nnconv_bf16w: width 64 only")
    y = out if out is not None else torch.empty_like(x)
    check(lib.mdno_nnconv_bf16w_fwd(ptr(x), ptr(graph.row_ptr), ptr(graph.src), x.shape[0], ptr(w_e),
                                    ptr(f32(root)) if root is not None else None,
                                    ptr(f32(bias)) if bias is not None else None, AGGR[aggr], int(relu), ptr(y),
                                    stream_ptr(x.device)), "mdno_nnconv_bf16w_fwd")
    return y


def nnconv_bwd_x_bf16w(gz: torch.Tensor, gs: torch.Tensor, by_src: CSRGraph, w_e: torch.Tensor, root) -> torch.Tensor:
    return _nnconv_bwd_x(gz, gs, by_src, w_e, root, bf16w=True)


def nnconv_bwd_we_bf16(x_layers: torch.Tensor, gs_layers: torch.Tensor, graph: CSRGraph, with_colsum: bool = False):
    """d_we bf16 [E,4096] (and the fp32 column sums of the rounded values): see `_nnconv_bwd_we`."""
    return _nnconv_bwd_we(x_layers, gs_layers, graph, with_colsum, bf16=True)


def relu_bwd_bf16(g: torch.Tensor, y: torch.Tensor, out_bf16: bool = True) -> torch.Tensor:
    lib = _lib.load()
    g, y = f32(g), _bf16(y)
    rows, n = g.shape
    out = torch.empty((rows, n), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=g.device)
    check(lib.mdno_relu_bwd_bf16(ptr(g), ptr(y), rows, n, int(out_bf16), ptr(out), stream_ptr(g.device)),
          "mdno_relu_bwd_bf16")
    return out


def colsum_bf16(a: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a = _bf16(a)
    rows, n = a.shape
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    ws = _ws(lib.mdno_colsum_bf16_workspace_bytes(n), a.device)
    check(lib.mdno_colsum_bf16(ptr(a), rows, n, ptr(out), ptr(ws), ws.numel(), stream_ptr(a.device)), "mdno_colsum_bf16")
    return out


def _check_chain(what: str, x_layers: torch.Tensor, layers: int, w_e: torch.Tensor, *params) -> None:
    """The chain entries are 64x64 only and read every operand at that size: refuse any other shape before a launch
    (a [R,1] stack or a [E,1] W_e would otherwise be read as [R,64] / [E,4096])."""
    if layers < 3:
        raise MdnoError(f"{what}: depth must be >= 1 (x_layers needs 2*depth+1 >= 3 layers)")
    if x_layers.dim() != 3 or x_layers.shape[0] != layers or x_layers.shape[2] != 64:
        raise MdnoError(f"{what}: x_layers {tuple(x_layers.shape)}, expected [{layers}, R, 64]")
    if w_e.dim() != 2 or w_e.shape[1] != 4096:
        raise MdnoError(f"{what}: w_e {tuple(w_e.shape)}, expected [E, 4096] (64x64 channels only)")
    for t in params:
        want = (64, 64) if t.dim() == 2 else (64,)
        if tuple(t.shape) != want:
            raise MdnoError(f"{what}: root/bias {tuple(t.shape)}, expected {want}")


def nnconv_chain_fwd(x_layers: torch.Tensor, graph: CSRGraph, w_e: torch.Tensor, root1, bias1, root2, bias2,
                     depth: int) -> None:
    """x_layers f32 [2*depth+1, R, 64]: [0] given, [a] = relu(conv(x[a-1])) written in place — the 2*depth conv
    applications of the block in one call (w_e fp32 or bf16 [E,4096])."""
    _check_chain("nnconv_chain_fwd", x_layers, 2 * depth + 1, w_e, root1, root2, bias1, bias2)
    lib = _lib.load()
    R = x_layers.shape[1]
    args = (ptr(x_layers), ptr(graph.row_ptr), ptr(graph.src), R, ptr(w_e), ptr(f32(root1)), ptr(f32(bias1)),
            ptr(f32(root2)), ptr(f32(bias2)), int(depth), stream_ptr(x_layers.device))
    if w_e.dtype == torch.bfloat16:
        check(lib.mdno_nnconv_chain_bf16w_fwd(*args), "mdno_nnconv_chain_bf16w_fwd")
    else:
        check(lib.mdno_nnconv_chain_fwd(*args), "mdno_nnconv_chain_fwd")


def nnconv_chain_bwd(g_out: torch.Tensor, x_layers: torch.Tensor, inv_deg: torch.Tensor, by_src: CSRGraph,
                     w_e: torch.Tensor, root1, root2, depth: int):
    """Backward through the 2*depth applications -> (gz [L,R,64], gs [L,R,64], g_in [R,64])."""
    _check_chain("nnconv_chain_bwd", x_layers, 2 * depth + 1, w_e, root1, root2)
    if tuple(g_out.shape) != tuple(x_layers.shape[1:]):
        raise MdnoError(f"nnconv_chain_bwd: g_out {tuple(g_out.shape)} != {tuple(x_layers.shape[1:])}")
    lib = _lib.load()
    L, R = 2 * depth, x_layers.shape[1]
    dev = x_layers.device
    gz = torch.empty((L, R, 64), dtype=torch.float32, device=dev)
    gs = torch.empty((L, R, 64), dtype=torch.float32, device=dev)
    g_in = torch.empty((R, 64), dtype=torch.float32, device=dev)
    args = (ptr(f32(g_out)), ptr(x_layers), ptr(inv_deg), ptr(by_src.row_ptr), ptr(by_src.perm), ptr(by_src.src), R,
            ptr(w_e), ptr(f32(root1)), ptr(f32(root2)), int(depth), ptr(gz), ptr(gs), ptr(g_in), stream_ptr(dev))
    if w_e.dtype == torch.bfloat16:
        check(lib.mdno_nnconv_chain_bf16w_bwd(*args), "mdno_nnconv_chain_bf16w_bwd")
    else:
        check(lib.mdno_nnconv_chain_bwd(*args), "mdno_nnconv_chain_bwd")
    return gz, gs, g_in


def train_moment_fwd(x_layers: torch.Tensor, graph: CSRGraph, edge_attr: torch.Tensor, weights, root1, bias1, root2, bias2,
                     depth: int, gemm_mode: str) -> torch.Tensor:
    """Forward of the kernel-integral block in the factored formulation (include/mdno_train.h mdno_train_moment_fwd):
    x_layers f32 [2*depth+1, R, 64] with layer 0 given, layers 1.. written in place; `edge_attr` [E, ker_in] in the
    caller's edge order (graph.perm maps it to CSR order), `weights` = (w0, b0, w1, b1, w2, b2).  Returns the edge-MLP's
    last hidden activation H as the k-tiled image the backward reads again."""
    lib = _lib.load()
    L = 2 * depth
    if x_layers.dim() != 3 or x_layers.shape[0] != L + 1 or x_layers.shape[2] != 64 or depth < 1:
        raise MdnoError(f"train_moment_fwd: x_layers {tuple(x_layers.shape)}, expected [{L + 1}, R, 64] with depth >= 1")
    w = [f32(t) for t in weights]
    k, ker_in = w[2].shape[0], w[0].shape[1]
    if tuple(w[4].shape) != (4096, k) or tuple(w[2].shape) != (k, k):
        raise MdnoError(f"train_moment_fwd: edge-MLP shapes {[tuple(t.shape) for t in w]} (width 64 only)")
    dev, R = x_layers.device, x_layers.shape[1]
    ea = f32(edge_attr)
    E = graph.edge_count()
    if ea.shape[0] != E or ea.dim() != 2 or ea.shape[1] != ker_in:
        raise MdnoError(f"train_moment_fwd: edge_attr {tuple(ea.shape)}, expected [{E}, {ker_in}]")
    if E == 0:                  # (never read: the device edge count is 0; the pointer must not be null)
        ea = torch.zeros((1, ker_in), dtype=torch.float32, device=dev)
    mode = _lib.GEMM_MODES[gemm_mode]
    h_img = torch.empty(lib.mdno_train_moment_h_floats(E, k), dtype=torch.float32, device=dev)
    ws = _ws(lib.mdno_train_moment_fwd_workspace_bytes(R, k, graph.edge_cap, mode), dev)
    check(lib.mdno_train_moment_fwd(ptr(ea), ptr(graph.perm), ptr(graph.num_edges), graph.edge_cap, ker_in, k, mode,
                                    *[ptr(t) for t in w], ptr(graph.row_ptr), ptr(graph.src), ptr(graph.dst), R,
                                    ptr(f32(root1)), ptr(f32(bias1)), ptr(f32(root2)), ptr(f32(bias2)), int(depth),
                                    ptr(x_layers), ptr(h_img), ptr(ws), ws.numel(), stream_ptr(dev)), "mdno_train_moment_fwd")
    return h_img


def train_moment_bwd(g_out: torch.Tensor, x_layers: torch.Tensor, h_img: torch.Tensor, graph: CSRGraph, by_src: CSRGraph,
                     w2: torch.Tensor, b2: torch.Tensor, root1, root2, depth: int, gemm_mode: str):
    """Backward through the 2*depth factored applications (mdno_train_moment_bwd) ->
    (gz [L,R,64], g_in [R,64], gz2 [E,k] = (H > 0) * dLoss/dH row-major, d_w2 [4096,k], d_b2 [4096])."""
    lib = _lib.load()
    L, R = 2 * depth, x_layers.shape[1]
    if tuple(g_out.shape) != (R, 64) or x_layers.shape[0] != L + 1:
        raise MdnoError(f"train_moment_bwd: g_out {tuple(g_out.shape)}, x_layers {tuple(x_layers.shape)}")
    w2, b2 = f32(w2), f32(b2)
    k = w2.shape[1]
    E = graph.edge_count()
    dev = x_layers.device
    if h_img.numel() != lib.mdno_train_moment_h_floats(E, k):
        raise MdnoError(f"train_moment_bwd: H image of {h_img.numel()} floats for {E} edges, k = {k}")
    gz = torch.empty((L, R, 64), dtype=torch.float32, device=dev)
    g_in = torch.empty((R, 64), dtype=torch.float32, device=dev)
    gz2 = torch.empty((E, k), dtype=torch.float32, device=dev)
    d_w2 = torch.empty((4096, k), dtype=torch.float32, device=dev)
    d_b2 = torch.empty(4096, dtype=torch.float32, device=dev)
    ws = _ws(lib.mdno_train_moment_bwd_workspace_bytes(R, k, E), dev)
    gz2_arg = gz2 if E else torch.empty((1, k), dtype=torch.float32, device=dev)
    check(lib.mdno_train_moment_bwd(ptr(f32(g_out)), ptr(x_layers), ptr(h_img), ptr(graph.row_ptr), ptr(graph.src),
                                    ptr(by_src.row_ptr), ptr(by_src.perm), R, E, k, int(depth), _lib.GEMM_MODES[gemm_mode],
                                    ptr(w2), ptr(b2), ptr(f32(root1)), ptr(f32(root2)), ptr(gz), ptr(g_in), ptr(gz2_arg),
                                    ptr(d_w2), ptr(d_b2), ptr(ws), ws.numel(), stream_ptr(dev)), "mdno_train_moment_bwd")
    return gz, g_in, gz2, d_w2, d_b2


def colsum_atb_bf16(a: torch.Tensor, b: torch.Tensor):
    """(column sums of a bf16 [rows,n], a^T . b for b fp32 [rows,6 or 8]) in one pass over a -> ([n], [n,kb]);
    other shapes: the two separate ops."""
    lib = _lib.load()
    a, b = _bf16(a), f32(b)
    rows, n = a.shape
    kb = b.shape[1]
    if kb not in (6, 8) or n % 8:
        pad = torch.zeros((rows, 128), dtype=torch.float32, device=a.device)
        pad[:, :kb].copy_(b)
        return colsum_bf16(a), gemm_atb_bf16(a, cast_bf16(pad))[:, :kb].contiguous()
    colsum = torch.empty(n, dtype=torch.float32, device=a.device)
    atb = torch.empty((n, kb), dtype=torch.float32, device=a.device)
    ws = _ws(lib.mdno_colsum_atb_bf16_workspace_bytes(n, kb), a.device)
    check(lib.mdno_colsum_atb_bf16(ptr(a), ptr(b), rows, n, kb, ptr(colsum), ptr(atb), ptr(ws), ws.numel(),
                                   stream_ptr(a.device)), "mdno_colsum_atb_bf16")
    return colsum, atb


# ------------------------------------------------------------------------------------------------
# Per-atom ends (node prologue, fc2) forward + backward for training (include/mdno.h, csrc/train_nodes.hip)
def fc_out(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """x . w^T + b  (fc2, graph_kernel.py:305): x [rows,width], w [out_width,width]."""
    lib = _lib.load()
    x, w = f32(x), f32(w)
    rows, width = x.shape
    ow = w.shape[0]
    out = torch.empty((rows, ow), dtype=torch.float32, device=x.device)
    check(lib.mdno_fc_out_fwd(ptr(x), ptr(w), ptr(f32(b)) if b is not None else None, rows, width, ow, ptr(out),
                              stream_ptr(x.device)), "mdno_fc_out_fwd")
    return out


def fc_out_bwd(x: torch.Tensor, w: torch.Tensor, g: torch.Tensor):
    """-> (dx [rows,width], d_w [out_width,width], d_b [out_width])"""
    lib = _lib.load()
    x, w, g = f32(x), f32(w), f32(g)
    rows, width = x.shape
    ow = w.shape[0]
    dx = torch.empty_like(x)
    d_w = torch.empty_like(w)
    d_b = torch.empty(ow, dtype=torch.float32, device=x.device)
    ws = _ws(lib.mdno_fc_out_bwd_workspace_bytes(rows, width, ow), x.device)
    check(lib.mdno_fc_out_bwd(ptr(x), ptr(w), ptr(g), rows, width, ow, ptr(dx), ptr(d_w), ptr(d_b), ptr(ws), ws.numel(),
                              stream_ptr(x.device)), "mdno_fc_out_bwd")
    return dx, d_w, d_b


def node_prologue_bwd(pack: ParamPack, frames: torch.Tensor, x_aminoacid: torch.Tensor, x0: torch.Tensor,
                      g0: torch.Tensor, need_frames: bool = False):
    """Backward of `node_prologue`: -> dict of gradients under the state_dict key names; `need_frames`: also
    dLoss/dframes f32 [W,M,N,3] under "frames" (include/mdno_unroll.h mdno_node_prologue_bwd_frames: the same launches,
    the same parameter gradients bit for bit)."""
    lib = _lib.load()
    frames = f32(frames)
    if frames.dim() == 3:
        frames = frames.unsqueeze(1)
    W, M, N, _ = frames.shape
    dev = frames.device
    aa = x_aminoacid.to(device=dev, dtype=torch.long).contiguous()
    p = pack.struct
    has_lstm = "lstm_w_ih" in pack.tensors
    d_lstm = torch.empty(108, dtype=torch.float32, device=dev) if has_lstm else None
    d_emb = torch.empty((p.num_embeddings, p.embedding_dim), dtype=torch.float32, device=dev)
    emb_out = d_emb if d_emb.numel() else torch.empty(1, dtype=torch.float32, device=dev)     # (embedding_dim 0)
    d_w = torch.empty((p.width, p.in_width), dtype=torch.float32, device=dev)
    d_b = torch.empty(p.width, dtype=torch.float32, device=dev)
    ws = _ws(lib.mdno_node_prologue_bwd_workspace_bytes(pack.ref, M * N), dev)
    if need_frames:
        d_frames = torch.empty_like(frames)
        check(lib.mdno_node_prologue_bwd_frames(pack.ref, ptr(frames), M, W, N, ptr(aa), int(aa.numel() == M * N and M > 1),
                                                ptr(f32(x0)), ptr(f32(g0)), ptr(d_lstm), ptr(emb_out), ptr(d_w), ptr(d_b),
                                                ptr(d_frames), ptr(ws), ws.numel(), stream_ptr(dev)),
              "mdno_node_prologue_bwd_frames")
    else:
        check(lib.mdno_node_prologue_bwd(pack.ref, ptr(frames), M, W, N, ptr(aa), int(aa.numel() == M * N and M > 1),
                                         ptr(f32(x0)), ptr(f32(g0)), ptr(d_lstm), ptr(emb_out), ptr(d_w), ptr(d_b), ptr(ws),
                                         ws.numel(), stream_ptr(dev)), "mdno_node_prologue_bwd")
    out = {"emb.weight": d_emb, "fc1.weight": d_w, "fc1.bias": d_b}
    if need_frames:
        out["frames"] = d_frames
    if has_lstm:
        # six DISJOINT slices of one buffer (the kernel writes b_hh's gradient — the same values as b_ih's — a second
        # time at [96:108]): autograd's AccumulateGrad keeps the tensor it is handed, so no two .grad tensors may
        # share memory (clip_grad_norm_, accumulation without zero_grad), and none of them needs a copy
        out.update({"lstm.weight_ih_l0": d_lstm[0:36].view(12, 3), "lstm.weight_hh_l0": d_lstm[36:72].view(12, 3),
                    "lstm.bias_ih_l0": d_lstm[72:84], "lstm.bias_hh_l0": d_lstm[96:108],
                    "lstm_fc.weight": d_lstm[84:93].view(3, 3), "lstm_fc.bias": d_lstm[93:96]})
    return out


# ------------------------------------------------------------------------------------------------
def collate_samples(pos: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor, meta: torch.Tensor, B: int, N: int,
                    W: int, horizon: int, n_edges: int, max_edges_per_sample: int):
    """Block-diagonal training batch built on the device (include/mdno.h mdno_collate_samples).
    -> (x_position [W,B*N,3], y [B*N,3], edge_index i64 [2,E], edge_attr [E,6])"""
    lib = _lib.load()
    dev = pos.device
    x_position = torch.empty((W, B * N, 3), dtype=torch.float32, device=dev)
    y = torch.empty((B * N, 3), dtype=torch.float32, device=dev)
    edge_index = torch.empty((2, n_edges), dtype=torch.long, device=dev)
    edge_attr = torch.empty((n_edges, 6), dtype=torch.float32, device=dev)
    check(lib.mdno_collate_samples(ptr(pos), ptr(rows), ptr(cols), ptr(meta), B, N, W, horizon, max_edges_per_sample,
                                   ptr(x_position), ptr(y), ptr(edge_index), ptr(edge_attr), stream_ptr(dev)),
          "mdno_collate_samples")
    return x_position, y, edge_index, edge_attr


def collate_positions(pos: torch.Tensor, meta: torch.Tensor, B: int, N: int, W: int, horizon: int):
    """The positions launch of mdno_collate_samples alone (max_edges_per_sample = 0: its edge launch does not run) ->
    (x_position [W,B*N,3], y [B*N,3]) — for batches whose edges do not come from a stored list (a periodic
    DeviceTrajectory).  The edge arguments are one small buffer nothing reads or writes: the entry refuses null."""
    lib = _lib.load()
    dev = pos.device
    x_position = torch.empty((W, B * N, 3), dtype=torch.float32, device=dev)
    y = torch.empty((B * N, 3), dtype=torch.float32, device=dev)
    unused = torch.empty(8, dtype=torch.int64, device=dev)
    check(lib.mdno_collate_samples(ptr(pos), ptr(unused), ptr(unused), ptr(meta), B, N, W, horizon, 0, ptr(x_position),
                                   ptr(y), ptr(unused), ptr(unused), stream_ptr(dev)), "mdno_collate_samples")
    return x_position, y


def collate_targets(pos: torch.Tensor, meta: torch.Tensor, B: int, N: int, W: int, horizon: int, steps: int) -> torch.Tensor:
    """Targets of an unrolled step (include/mdno_unroll.h mdno_collate_targets): y f32 [steps, B*N, 3], step k of sample
    b = frame meta[b] + W + horizon - 1 + k of the resident trajectory `pos` [T,N,3]; one launch."""
    lib = _lib.load()
    if int(steps) < 1:
        raise MdnoError(f"collate_targets: steps={steps} (>= 1)")
    y = torch.empty((int(steps), B * N, 3), dtype=torch.float32, device=pos.device)
    check(lib.mdno_collate_targets(ptr(pos), int(pos.shape[0]), ptr(meta), B, N, W, horizon, int(steps), ptr(y),
                                   stream_ptr(pos.device)), "mdno_collate_targets")
    return y


# ------------------------------------------------------------------------------------------------
# Gradients with respect to the model's inputs (include/mdno_unroll.h, csrc/input_grad.hip)
def edge_mlp_input_bwd(gz1: torch.Tensor, w0: torch.Tensor, num_edges: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_edge_attr f32 [rows, ker_in] = gz1 [rows, k] . w0 [k, ker_in] for the first `num_edges` (i32 [1], device) rows,
    in gz1's (CSR) edge order; rows past the count are left as they are (`out`: the buffer to write, else a new one)."""
    lib = _lib.load()
    gz1, w0 = f32(gz1), f32(w0)
    rows, k = gz1.shape
    ker_in = w0.shape[1]
    if w0.shape[0] != k or not 1 <= ker_in <= 8:
        raise MdnoError(f"edge_mlp_input_bwd: gz1 {tuple(gz1.shape)}, w0 {tuple(w0.shape)} (ker_in 1..8)")
    if out is None:
        out = torch.empty((rows, ker_in), dtype=torch.float32, device=gz1.device)
    elif tuple(out.shape) != (rows, ker_in) or out.dtype != torch.float32:
        raise MdnoError(f"edge_mlp_input_bwd: out must be f32 {(rows, ker_in)}")
    if rows == 0:
        return out
    check(lib.mdno_edge_mlp_input_bwd(ptr(gz1), ptr(w0), ptr(num_edges), rows, k, ker_in, ptr(out), stream_ptr(gz1.device)),
          "mdno_edge_mlp_input_bwd")
    return out


def edge_attr_from_pos(pos: torch.Tensor, graph: CSRGraph, box=None, cutoff: float = 8.0) -> torch.Tensor:
    """edge_attr f32 [E, 6] = [pos[src p], pos[dst p]] in the graph's CSR edge order (mdno_edge_attr_from_pos): the
    attributes the forward forms from `edge_pos` for the same graph.
    `box` = (Lx, Ly, Lz) with a periodic axis: the source is moved to its minimum image next to the destination
    (include/mdno_pbc_train.h mdnopbt_edge_attr_from_pos; `cutoff` only validates the box, as everywhere) — on a graph
    from `radius_graph_pbc` of the same positions, the rows that call wrote, bit for bit.  box None or all zero: the
    open call, untouched."""
    box = check_box(box, cutoff)
    lib = _lib.load()
    pos = f32(pos).reshape(-1, 3)
    E = graph.edge_count()
    ea = torch.empty((E, 6), dtype=torch.float32, device=pos.device)
    if box is not None:
        if E:
            b = box_arg(box)
            check(lib.mdnopbt_edge_attr_from_pos(ptr(pos), ptr(graph.src), ptr(graph.dst), ptr(graph.num_edges), E,
                                                 pos.shape[0], float(cutoff), b, ptr(ea), stream_ptr(pos.device)),
                  "mdnopbt_edge_attr_from_pos")
        return ea
    if E:
        check(lib.mdno_edge_attr_from_pos(ptr(pos), ptr(graph.src), ptr(graph.dst), ptr(graph.num_edges), E, pos.shape[0],
                                          ptr(ea), stream_ptr(pos.device)), "mdno_edge_attr_from_pos")
    return ea


def edge_attr_pos_bwd(d_edge_attr: torch.Tensor, graph: CSRGraph, by_src: CSRGraph, num_rows: int) -> torch.Tensor:
    """The adjoint of `edge_attr_from_pos` (mdno_edge_attr_pos_bwd): d_pos f32 [num_rows, 3]; `by_src` =
    `source_sorted(graph, num_rows)`."""
    lib = _lib.load()
    g = f32(d_edge_attr)
    E = graph.edge_count()
    if g.dim() != 2 or tuple(g.shape) != (E, 6):
        raise MdnoError(f"edge_attr_pos_bwd: d_edge_attr {tuple(g.shape)}, expected {(E, 6)}")
    d_pos = torch.empty((num_rows, 3), dtype=torch.float32, device=g.device)
    if E == 0:                  # (never read: both row-pointer arrays end at 0; the pointer must not be null)
        g = torch.zeros((1, 6), dtype=torch.float32, device=g.device)
    check(lib.mdno_edge_attr_pos_bwd(ptr(g), ptr(graph.row_ptr), ptr(by_src.row_ptr), ptr(by_src.perm), int(num_rows),
                                     ptr(d_pos), stream_ptr(g.device)), "mdno_edge_attr_pos_bwd")
    return d_pos


# ------------------------------------------------------------------------------------------------
def _noise_seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise MdnoError(f"noise seed {seed} outside [0, 2^64)")
    return seed


def _noise_ids(ids, dev, what: str) -> torch.Tensor:
    """Stream ids (members, sample indices) as the int32 device vector the kernels read."""
    t = torch.as_tensor(ids).reshape(-1)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise MdnoError(f"{what} must be integers")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) > INT_MAX):
        raise MdnoError(f"{what} must lie in [0, 2^31)")
    return t.to(device=dev, dtype=torch.int32).contiguous()


def noise_fill(seed: int, stream_ids, index: int, n_atoms: int, frames: int = 1, purpose="rollout", sigma: float = 1.0,
               device=None, with_words: bool = False):
    """The raw generator (include/mdno_noise.h mdno_noise_fill; csrc/philox.h): sigma * z for every stream of
    `stream_ids` (ints or an integer tensor [M]) at `index` (step or epoch, < 2^48) -> f32 [M, frames * n_atoms * 3],
    element (frame * n_atoms + atom) * 3 + component; with `with_words` also the two Philox words behind every value,
    u32 as int64 [M, elems, 2].  purpose: "rollout" / "train_window" (or its number)."""
    lib = _lib.load()
    dev = _lib.require_gpu(device)
    ids = _noise_ids(stream_ids, dev, "stream_ids")
    M, E = int(ids.numel()), int(frames) * int(n_atoms) * 3
    if isinstance(purpose, str):
        if purpose not in _lib.NOISE_PURPOSES:
            raise MdnoError(f"purpose={purpose!r}: expected one of {sorted(_lib.NOISE_PURPOSES)} or a number in [0, 256)")
        purpose = _lib.NOISE_PURPOSES[purpose]
    if not isinstance(purpose, int) or isinstance(purpose, bool) or not 0 <= purpose < 256:
        raise MdnoError(f"purpose={purpose!r}: expected one of {sorted(_lib.NOISE_PURPOSES)} or a number in [0, 256)")
    z = torch.empty((M, E), dtype=torch.float32, device=dev)
    words = torch.empty((M, E, 2), dtype=torch.int32, device=dev) if with_words else None
    check(lib.mdno_noise_fill(_noise_seed(seed), ptr(ids), M, int(index), int(n_atoms), E,
                              purpose, float(sigma), ptr(z), ptr(words), stream_ptr(dev)),
          "mdno_noise_fill")
    if with_words:
        return z, words.to(torch.int64) & 0xFFFFFFFF
    return z


def noise_add_window(x_position: torch.Tensor, sample_ids, row_offsets: torch.Tensor, max_rows: int, sigma: float,
                     seed: int, epoch: int) -> torch.Tensor:
    """x_position f32 [W, R, 3] of a collated batch + sigma * z, as a new tensor (include/mdno_noise.h
    mdno_noise_add_window): sample b owns rows row_offsets[b] .. row_offsets[b+1]-1 (i32 [B+1] on the device) and draws
    from stream sample_ids[b] (its index in the dataset) at index `epoch`."""
    lib = _lib.load()
    x = f32(x_position)
    dev = x.device
    if x.dim() != 3 or x.shape[2] != 3:
        raise MdnoError(f"x_position shape {tuple(x.shape)}: expected [W, R, 3]")
    ids = _noise_ids(sample_ids, dev, "sample_ids")
    B = int(ids.numel())
    if row_offsets.dtype != torch.int32 or row_offsets.numel() != B + 1:
        raise MdnoError("row_offsets must be int32 [B + 1]")
    out = torch.empty_like(x)
    check(lib.mdno_noise_add_window(_noise_seed(seed), ptr(ids), ptr(row_offsets), B, int(x.shape[0]), int(x.shape[1]),
                                    int(max_rows), int(epoch), float(sigma), ptr(x), ptr(out), stream_ptr(dev)),
          "mdno_noise_add_window")
    return out


# ------------------------------------------------------------------------------------------------
# Random rigid motions of training samples (include/mdno_augment.h, csrc/rigid_rule.h, csrc/augment.hip)
def rigid_motions(seed: int, sample_ids, epoch: int, rotate: bool = True, translate: float = 0.0,
                  last_element: int = _lib.AUGMENT_LAST_ELEMENT, first_frame: Optional[torch.Tensor] = None,
                  n_atoms: Optional[int] = None, device=None):
    """One rigid motion per sample of `sample_ids` (ints or an integer tensor [B]: indices in the dataset), keyed by
    (seed, sample, epoch) alone (mdnoaug_motions) -> (quaternion f64 [B,4] as (w,x,y,z), pivot f64 [B,3], shift f64 [B,3],
    attempts i32 [B,2]).  An int32 tensor already on the device is taken as it is (no read-back to check its range).
    first_frame f32 [B * n_atoms, 3]: the pivot is every sample's centroid in it; None: the origin.
    last_element < 65 shortens the rejection loop (tests reach the identity fallback with it)."""
    seed, epoch, last_element, translate = _noise_seed(seed), int(epoch), int(last_element), float(translate)
    integer(last_element, "last_element", 2, _lib.AUGMENT_LAST_ELEMENT)
    real(translate, "translate", positive=False)
    integer(epoch, "epoch", 0, 2 ** 48 - 1)
    B = int(torch.as_tensor(sample_ids).numel())
    if first_frame is not None:
        n_atoms = int(n_atoms) if n_atoms is not None else 0
        if n_atoms < 1 or first_frame.dim() != 2 or tuple(first_frame.shape) != (B * n_atoms, 3):
            raise MdnoError(f"first_frame shape {tuple(first_frame.shape)}: expected [B * n_atoms, 3] = [{B * n_atoms}, 3]")
        device = first_frame.device if device is None else device
    lib = _lib.load()
    dev = _lib.require_gpu(device)
    if torch.is_tensor(sample_ids) and sample_ids.dtype == torch.int32 and sample_ids.device == dev:
        ids = sample_ids.reshape(-1).contiguous()
    else:
        ids = _noise_ids(sample_ids, dev, "sample_ids")
    frame = None if first_frame is None else f32(first_frame)
    q = torch.empty((B, 4), dtype=torch.float64, device=dev)
    pivot = torch.empty((B, 3), dtype=torch.float64, device=dev)
    shift = torch.empty((B, 3), dtype=torch.float64, device=dev)
    attempts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    check(lib.mdnoaug_motions(seed, ptr(ids), B, epoch, int(bool(rotate)), translate, last_element, ptr(frame),
                              int(n_atoms or 0), ptr(q), ptr(pivot), ptr(shift), ptr(attempts), stream_ptr(dev)),
          "mdnoaug_motions")
    return q, pivot, shift, attempts


def rigid_apply(quaternion: torch.Tensor, pivot: torch.Tensor, shift: torch.Tensor, n_atoms: int, rows: torch.Tensor,
                inverse: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The motions (inverse: their inverses) of `rows` f32 [..., B * N, 3] (mdnoaug_apply): sample b owns rows
    b * N .. b * N + N - 1 of every frame.  A new tensor, or `out` (which may be `rows`: in place)."""
    B, N = int(quaternion.shape[0]), int(n_atoms)
    if tuple(quaternion.shape) != (B, 4) or tuple(pivot.shape) != (B, 3) or tuple(shift.shape) != (B, 3) or \
            any(t.dtype != torch.float64 for t in (quaternion, pivot, shift)):
        raise MdnoError("quaternion [B, 4], pivot [B, 3] and shift [B, 3] must be float64")
    if rows.dim() < 2 or rows.shape[-1] != 3 or rows.shape[-2] != B * N:
        raise MdnoError(f"rows shape {tuple(rows.shape)}: expected [..., B * N, 3] with B * N = {B} * {N}")
    x = f32(rows)
    if out is not None:
        operand(out, "out", torch.float32, tuple(x.shape), x.device)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    F = x.numel() // max(B * N * 3, 1)
    check(lib.mdnoaug_apply(ptr(quaternion), ptr(pivot), ptr(shift), B, N, F, int(bool(inverse)), ptr(x), ptr(out),
                            stream_ptr(x.device)), "mdnoaug_apply")
    return out


def edge_attr_gather(x0: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
    """edge_attr f32 [E, 6] of a collated batch gathered again from its first window frame x0 f32 [R, 3]
    (mdnoaug_edge_attr): row e = (x0[edge_index[0][e]], x0[edge_index[1][e]]), NaN where an index lies outside [0, R)."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise MdnoError(f"edge_index shape {tuple(edge_index.shape)}: expected [2, E]")
    if edge_index.dtype != torch.int64:
        raise MdnoError(f"edge_index must be int64 (got {edge_index.dtype})")
    if x0.dim() != 2 or x0.shape[1] != 3:
        raise MdnoError(f"x0 shape {tuple(x0.shape)}: expected [R, 3]")
    lib = _lib.load()
    x = f32(x0)
    E = int(edge_index.shape[1])
    out = torch.empty((E, 6), dtype=torch.float32, device=x.device)
    check(lib.mdnoaug_edge_attr(ptr(x), ptr(edge_index), E, int(x.shape[0]), ptr(out), stream_ptr(x.device)),
          "mdnoaug_edge_attr")
    return out


# ------------------------------------------------------------------------------------------------
def lploss_rel_fwd(out: torch.Tensor, y: torch.Tensor, size_average: bool):
    """LpLoss.rel, p = 2, and the batch MSE in one pass (include/mdno.h mdno_lploss_rel_fwd): out, y f32 [B, D] ->
    (loss_mse f32 [2] = [loss, mse], stats f32 [B, 4] for the backward)."""
    lib = _lib.load()
    out, y = f32(out), f32(y)
    if out.dim() != 2 or out.shape != y.shape:
        raise MdnoError(f"lploss_rel: out {tuple(out.shape)} and y {tuple(y.shape)} must be the same [B, D]")
    B, D = out.shape
    stats = torch.empty((B, 4), dtype=torch.float32, device=out.device)
    res = torch.empty(2, dtype=torch.float32, device=out.device)
    check(lib.mdno_lploss_rel_fwd(ptr(out), ptr(y), B, D, int(bool(size_average)), ptr(stats), ptr(res),
                                  stream_ptr(out.device)), "mdno_lploss_rel_fwd")
    return res, stats


def lploss_rel_bwd(out: torch.Tensor, y: torch.Tensor, stats: torch.Tensor, grad_loss, size_average: bool) -> torch.Tensor:
    """d loss / d out (include/mdno.h mdno_lploss_rel_bwd); grad_loss: the f32 scalar tensor autograd hands down, or None."""
    lib = _lib.load()
    B, D = out.shape
    g = torch.empty_like(out)
    gl = None if grad_loss is None else f32(grad_loss).reshape(1)
    check(lib.mdno_lploss_rel_bwd(ptr(out), ptr(y), ptr(stats), ptr(gl), B, D, int(bool(size_average)), ptr(g),
                                  stream_ptr(out.device)), "mdno_lploss_rel_bwd")
    return g


# ------------------------------------------------------------------------------------------------
# Backward of the stand-alone NNConv_old / DenseNet (include/mdno.h "Backward of the stand-alone layers",
# csrc/layer_grad.hip); graph_kernel.py's autograd Functions call these.
def nnconv_msg_grad(x: torch.Tensor, graph: CSRGraph, w_e: torch.Tensor, g: torch.Tensor, aggr: str) -> torch.Tensor:
    """gm f32 [E, Cout] = dLoss/dm_e in the graph's CSR edge order (max: ties share g evenly)."""
    lib = _lib.load()
    x, g = f32(x), f32(g)
    R, cin = x.shape
    cout = g.shape[1]
    gm = torch.empty((max(graph.edge_count(), 1), cout), dtype=torch.float32, device=x.device)
    check(lib.mdno_nnconv_msg_grad(ptr(x), ptr(graph.row_ptr), ptr(graph.src), R, ptr(w_e), ptr(g), cin, cout, AGGR[aggr],
                                   ptr(gm), stream_ptr(x.device)), "mdno_nnconv_msg_grad")
    return gm


def nnconv_bwd_x_edges(gm: torch.Tensor, g: torch.Tensor, by_src: CSRGraph, w_e: torch.Tensor,
                       root: Optional[torch.Tensor], cin: int) -> torch.Tensor:
    """dx [R, Cin] = g . root^T + sum over each row's out-edges of W_e . gm_e (any Cin, Cout)."""
    lib = _lib.load()
    g = f32(g)
    R, cout = g.shape
    dx = torch.empty((R, cin), dtype=torch.float32, device=g.device)
    check(lib.mdno_nnconv_bwd_x_edges(ptr(gm), ptr(g), ptr(by_src.row_ptr), ptr(by_src.perm), R, ptr(w_e),
                                      ptr(f32(root)) if root is not None else None, cin, cout, ptr(dx),
                                      stream_ptr(g.device)), "mdno_nnconv_bwd_x_edges")
    return dx


def nnconv_bwd_we_edges(x: torch.Tensor, gm: torch.Tensor, graph: CSRGraph) -> torch.Tensor:
    """d_we [E, Cin*Cout] = x[src e] (x) gm_e, CSR edge order."""
    lib = _lib.load()
    x = f32(x)
    R, cin = x.shape
    cout = gm.shape[1]
    e = graph.edge_count()
    d_we = torch.empty((e, cin * cout), dtype=torch.float32, device=x.device)
    if e > 0:
        check(lib.mdno_nnconv_bwd_we_edges(ptr(x), ptr(gm), ptr(graph.row_ptr), ptr(graph.src), R, cin, cout, ptr(d_we),
                                           stream_ptr(x.device)), "mdno_nnconv_bwd_we_edges")
    return d_we


def scale_rows(a: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a = f32(a)
    rows, n = a.shape
    out = torch.empty_like(a)
    check(lib.mdno_scale_rows(ptr(a), ptr(f32(scale)), rows, n, ptr(out), stream_ptr(a.device)), "mdno_scale_rows")
    return out


def relu_mask_bwd(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """g where y > 0, else 0 (any shape)."""
    lib = _lib.load()
    g, y = f32(g), f32(y)
    out = torch.empty_like(g)
    check(lib.mdno_relu_mask_bwd(ptr(g), ptr(y), g.numel(), ptr(out), stream_ptr(g.device)), "mdno_relu_mask_bwd")
    return out


def scatter_rows(x: torch.Tensor, perm: torch.Tensor, rows: int) -> torch.Tensor:
    """out[perm[p]] = x[p] for p < rows: the inverse of `permute_rows` (CSR order back to the input's edge order)."""
    lib = _lib.load()
    x = f32(x)
    out = torch.empty((rows,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    width = int(x[0].numel()) if x.shape[0] else 1
    check(lib.mdno_scatter_rows(ptr(x), ptr(perm), rows, width, ptr(out), stream_ptr(x.device)), "mdno_scatter_rows")
    return out


def nnconv_bwd(x: torch.Tensor, graph: CSRGraph, w_e: torch.Tensor, root: Optional[torch.Tensor], g: torch.Tensor,
               aggr: str, need=(True, True, True, True), generic: bool = False):
    """Gradients of y = nnconv(x, graph, w_e, root, bias, aggr) (relu off) for g = dLoss/dy ->
    (dx [R,Cin], d_we [E,Cin*Cout] in CSR order, d_root [Cin,Cout], d_bias [Cout]); an entry is None where `need` says
    so.  64x64 add / mean run the model's tuned training kernels (mdno_nnconv_bwd_x / _we with gs = g / max(deg, 1))
    unless `generic`; everything else goes through the per-edge message gradient (mdno_nnconv_msg_grad)."""
    x, g = f32(x), f32(g)
    R, cin = x.shape
    cout = g.shape[1]
    e = graph.edge_count()
    need_x, need_w, need_root, need_bias = need
    dx = d_we = d_root = d_bias = None
    by_src = source_sorted(graph, R) if need_x and e > 0 else None
    if e == 0:                  # no messages: dx = g . root^T, and W_e (no edge rows) gets a zero gradient
        if need_x:
            dx = linear(g, root, None) if root is not None else torch.zeros((R, cin), dtype=torch.float32,
                                                                            device=x.device)
        if need_w:
            d_we = torch.zeros_like(w_e)
    elif not generic and cin == 64 and cout == 64 and aggr in ("add", "mean"):
        gs = scale_rows(g, inv_degree(graph, aggr)) if aggr == "mean" else g
        if need_x:
            dx = nnconv_bwd_x(g, gs, by_src, w_e, root)
        if need_w:
            d_we = nnconv_bwd_we(x.unsqueeze(0), gs.unsqueeze(0), graph)
    elif need_x or need_w:
        gm = nnconv_msg_grad(x, graph, w_e, g, aggr)
        if need_x:
            dx = nnconv_bwd_x_edges(gm, g, by_src, w_e, root, cin)
        if need_w:
            d_we = nnconv_bwd_we_edges(x, gm, graph)
    if need_root and root is not None:
        d_root = gemm_atb(x, g)
    if need_bias:
        d_bias = colsum(g)
    return dx, d_we, d_root, d_bias


# ------------------------------------------------------------------------------------------------
# Scoring a rollout (include/mdno.h "Scoring a rollout", csrc/forecast.hip)
FORECAST_FORMS = {"auto": 0, "lds": 1, "tiled": 2}


def _device_frames(t, what: str, ranks) -> torch.Tensor:
    """`t` as a contiguous f32 device tensor [..., N, 3] of one of the given ranks, or MdnoError (no device work)."""
    return device_tensor(t, what, ranks, last=3)


def forecast_score(frames: torch.Tensor, truth: torch.Tensor, cutoff: float = 8.0, form: str = "auto", box=None):
    """frames f32 [S,M,N,3] against truth [S,N,3] (shared by the members) or [S,M,N,3] ->
    (mse f64 [S,M], rmsd f64 [S,M], counts i64 [S,M,3], first_nonfinite i32 [M]); mdno_forecast_score.  Asynchronous on
    the current stream, nothing is read back.  `form`: "auto" (one workgroup per (s, m) up to 2,048 atoms, tiled above),
    "lds" or "tiled" to force one (same counts; a test hook).  `box` = (Lx, Ly, Lz): contacts under the minimum-image
    rule of include/mdno_pbc.h (mdno_forecast_score_pbc); mse, rmsd and first_nonfinite do not depend on it."""
    box = check_box(box, cutoff)
    frames = _device_frames(frames, "frames", (4,))
    truth = _device_frames(truth, "truth", (3, 4))
    if truth.device != frames.device:
        raise MdnoError(f"truth is on {truth.device}, frames on {frames.device}")
    S, M, N, _ = frames.shape
    want = (S, M, N, 3) if truth.dim() == 4 else (S, N, 3)
    if tuple(truth.shape) != want:
        raise MdnoError(f"truth shape {tuple(truth.shape)} does not match frames {tuple(frames.shape)}: expected "
                        f"{(S, N, 3)} or {(S, M, N, 3)}")
    code = form_code(form, FORECAST_FORMS)
    lib = _lib.load()
    dev = frames.device
    scored = S * M > 0 and N > 0
    # (an (s, m) without atoms has no mean: NaN, and no contacts)
    mse = torch.empty((S, M), dtype=torch.float64, device=dev) if scored else \
        torch.full((S, M), float("nan"), dtype=torch.float64, device=dev)
    rmsd = torch.empty_like(mse) if scored else mse.clone()
    counts = torch.empty((S, M, 3), dtype=torch.int64, device=dev) if scored else \
        torch.zeros((S, M, 3), dtype=torch.int64, device=dev)
    first = torch.empty(M, dtype=torch.int32, device=dev)
    nbytes = lib.mdno_forecast_score_workspace_bytes(S, M, N, code)
    ws = _ws(nbytes, dev) if scored else None
    head = (ptr(frames) if scored else None, ptr(truth) if scored else None, int(truth.dim() == 4), S, M, N, float(cutoff))
    tail = (ptr(mse) if scored else None, ptr(rmsd) if scored else None, ptr(counts) if scored else None,
            ptr(first) if M else None, code, ptr(ws), ws.numel() if scored else 0, stream_ptr(dev))
    if box is None:
        check(lib.mdno_forecast_score(*head, *tail), "mdno_forecast_score")
    else:
        check(lib.mdno_forecast_score_pbc(*head, box_arg(box), *tail), "mdno_forecast_score_pbc")
    return mse, rmsd, counts, first


def contact_maps(frames: torch.Tensor, cutoff: float = 8.0, box=None) -> torch.Tensor:
    """frames f32 [..., N, 3] -> u8 [..., N, N], 1 where the pair is within `cutoff` (the radius graph's own test, self
    pairs included): the dense map get_contact_map (graph_kernel.py:416-424) builds.  mdno_contact_maps.  `box` =
    (Lx, Ly, Lz): the minimum-image test of include/mdno_pbc.h (mdno_contact_maps_pbc)."""
    box = check_box(box, cutoff)
    frames, lead, F, N = _flat_frames(frames)
    lib = _lib.load()
    maps = torch.empty(lead + (N, N), dtype=torch.uint8, device=frames.device)
    empty = F == 0 or N == 0
    if box is None:
        check(lib.mdno_contact_maps(None if empty else ptr(frames), F, N, float(cutoff), None if empty else ptr(maps),
                                    stream_ptr(frames.device)), "mdno_contact_maps")
    else:
        check(lib.mdno_contact_maps_pbc(None if empty else ptr(frames), F, N, float(cutoff), box_arg(box),
                                        None if empty else ptr(maps), stream_ptr(frames.device)), "mdno_contact_maps_pbc")
    return maps


# ------------------------------------------------------------------------------------------------
# Structural observables (include/mdno_observe.h, csrc/observe.hip)
MAX_HISTOGRAM_BINS = 4096


def check_histogram_args(r_max, n_bins, box=None):
    """(r_max as float, n_bins as int, box as check_box returns it) for a pair histogram, or MdnoError: r_max finite and
    > 0, n_bins in 1 .. 4096, every periodic axis of the box >= 2 * r_max (include/mdno_observe.h).  Host only."""
    r = real(r_max, "pair_histogram: r_max")
    return r, integer(n_bins, "pair_histogram: n_bins", 1, MAX_HISTOGRAM_BINS, exact=True), check_box(box, r)


def _flat_frames(frames):
    """(frames as contiguous f32 [..., N, 3] on the device, its leading shape, F, N), or MdnoError."""
    frames = _device_frames(frames, "frames", range(2, 9))
    lead = tuple(frames.shape[:-2])
    return frames, lead, math.prod(lead), frames.shape[-2]


def pair_histogram(frames: torch.Tensor, r_max: float, n_bins: int, box=None, form: str = "auto") -> torch.Tensor:
    """frames f32 [..., N, 3] -> i64 [..., n_bins]: per frame, the number of unordered pairs i < j whose distance lies
    in bin b of [0, r_max) (include/mdno_observe.h has the rule; mdno_pair_histogram).  `box` = (Lx, Ly, Lz), 0 for an
    open axis: distances by the minimum image, every periodic axis >= 2 * r_max.  Asynchronous on the current stream,
    nothing is read back.  `form`: "auto" (one workgroup per frame up to 2,048 atoms, pair tiles above), "lds" or
    "tiled" to force one (the same counts)."""
    r_max, n_bins, box = check_histogram_args(r_max, n_bins, box)
    code = form_code(form, FORECAST_FORMS)
    frames, lead, F, N = _flat_frames(frames)
    lib = _lib.load()
    dev = frames.device
    counts = torch.empty(lead + (n_bins,), dtype=torch.int64, device=dev)
    nbytes = lib.mdno_pair_histogram_workspace_bytes(F, N, n_bins, code)
    ws = _ws(nbytes, dev) if nbytes else None
    check(lib.mdno_pair_histogram(ptr(frames) if F * N else None, F, N, r_max, n_bins, box_arg(box) if box else None,
                                  ptr(counts) if F else None, code, ptr(ws), nbytes, stream_ptr(dev)),
          "mdno_pair_histogram")
    return counts


def radius_of_gyration(frames: torch.Tensor) -> torch.Tensor:
    """frames f32 [..., N, 3] -> f64 [...]: sqrt(mean_i |x_i - centroid|^2) per frame, two fixed-order fp64 passes
    (mdno_radius_of_gyration); NaN for a frame with a non-finite coordinate or without atoms."""
    frames, lead, F, N = _flat_frames(frames)
    lib = _lib.load()
    rg = torch.empty(lead, dtype=torch.float64, device=frames.device)
    check(lib.mdno_radius_of_gyration(ptr(frames) if F * N else None, F, N, ptr(rg) if F else None,
                                      stream_ptr(frames.device)), "mdno_radius_of_gyration")
    return rg


# ------------------------------------------------------------------------------------------------
# Time-correlation statistics (include/mdno_dynamics.h, csrc/dynamics.hip)
DYNAMICS_ORIGIN_CHUNK = 64          # MDNO_DYN_ORIGIN_CHUNK: origins per workgroup (fixes the order of the sums)
DYNAMICS_ATOM_TILE = 256            # MDNO_DYN_ATOM_TILE
MAX_LAGS = 1024


def _trajectory(frames, what: str = "frames"):
    """(frames as contiguous f32 [S, M, N, 3] on the device, S, M, N); [S, N, 3] is M = 1.  MdnoError otherwise."""
    frames = _device_frames(frames, what, (3, 4))
    if frames.dim() == 3:
        frames = frames[:, None]
    check_dims(what, frames.shape)
    return (frames, *frames.shape[:3])


def check_lags(lags, S: int, span: int = 0, what: str = "displacement_stats"):
    """`lags` as a list of Python ints: 1 .. 1024 integers in 0 .. S - 1 - span (include/mdno_dynamics.h), or MdnoError.
    Host only."""
    return int_list(lags, what, "lag", (1, MAX_LAGS), 0, S - 1 - span)


def check_origin_stride(origin_stride, what: str = "displacement_stats") -> int:
    return integer(origin_stride, f"{what}: origin_stride", 1, exact=True)


def n_origins(S: int, lag: int, origin_stride: int = 1, span: int = 0) -> int:
    """How many origins t = 0, stride, ... satisfy t + lag + span <= S - 1."""
    last = S - 1 - span - lag
    return 0 if last < 0 else last // origin_stride + 1


def _lag_arg(vals):
    return (C.c_int32 * len(vals))(*vals)


def displacement_stats(frames: torch.Tensor, lags, origin_stride: int = 1, remove_com: bool = False, r_max=None,
                       n_bins: int = 0):
    """frames f32 [S, M, N, 3] (or [S, N, 3]: M = 1) -> (sum2 f64 [M, L], sum4 f64 [M, L], counts i64 [M, L, n_bins] or
    None): per member and lag, the sums of |x_i(t + lag) - x_i(t)|^2 and of its square over all origins t = 0, stride, ...
    and atoms, and (n_bins > 0) the histogram of the displacements below r_max (include/mdno_dynamics.h has the rule;
    mdno_displacement_stats).  `remove_com`: the centroid's displacement is subtracted.  Fixed summation order: the same
    bits on every run.  Asynchronous on the current stream, nothing is read back."""
    frames, S, M, N = _trajectory(frames)
    stride = check_origin_stride(origin_stride)
    nb = integer(n_bins, "displacement_stats: n_bins", 0, MAX_HISTOGRAM_BINS, exact=True)
    r = real(r_max, f"displacement_stats: r_max (with n_bins={nb})") if nb > 0 else 0.0
    vals = check_lags(lags, S if S > 0 else 1 << 30)          # (no frames: any lag list of the right form passes)
    L = len(vals)
    lib = _lib.load()
    dev = frames.device
    sum2 = torch.empty((M, L), dtype=torch.float64, device=dev)
    sum4 = torch.empty((M, L), dtype=torch.float64, device=dev)
    counts = torch.empty((M, L, nb), dtype=torch.int64, device=dev) if nb > 0 else None
    if S == 0 or M == 0:
        return sum2.zero_(), sum4.zero_(), None if counts is None else counts.zero_()
    nbytes = lib.mdno_displacement_stats_workspace_bytes(S, M, N, L, nb)
    ws = _ws(nbytes, dev)
    check(lib.mdno_displacement_stats(ptr(frames) if N else None, S, M, N, _lag_arg(vals), L, stride, int(bool(remove_com)),
                                      r, nb, ptr(sum2), ptr(sum4), ptr(counts), ptr(ws), nbytes, stream_ptr(dev)),
          "mdno_displacement_stats")
    return sum2, sum4, counts


def velocity_autocorrelation(frames: torch.Tensor, lags, origin_stride: int = 1, remove_com: bool = False) -> torch.Tensor:
    """frames f32 [S, M, N, 3] (or [S, N, 3]) -> corr f64 [M, L]: the sum over origins and atoms of v_i(t) . v_i(t + lag)
    with the finite-difference velocities v(t) = x(t + 1) - x(t) (mdno_velocity_autocorrelation; lags in 0 .. S - 2).
    Same fixed order and stream behaviour as `displacement_stats`."""
    what = "velocity_autocorrelation"
    frames, S, M, N = _trajectory(frames)
    stride = check_origin_stride(origin_stride, what)
    vals = check_lags(lags, S if S > 0 else 1 << 30, 1, what)
    L = len(vals)
    lib = _lib.load()
    dev = frames.device
    corr = torch.empty((M, L), dtype=torch.float64, device=dev)
    if S == 0 or M == 0:
        return corr.zero_()
    nbytes = lib.mdno_velocity_autocorrelation_workspace_bytes(S, M, N, L)
    ws = _ws(nbytes, dev)
    check(lib.mdno_velocity_autocorrelation(ptr(frames) if N else None, S, M, N, _lag_arg(vals), L, stride,
                                            int(bool(remove_com)), ptr(corr), ptr(ws), nbytes, stream_ptr(dev)),
          "mdno_velocity_autocorrelation")
    return corr


def unwrap_frames(frames: torch.Tensor, box) -> torch.Tensor:
    """frames f32 [S, M, N, 3] or [S, N, 3] wrapped into the periodic cell `box` = (Lx, Ly, Lz) (0 = open axis) -> the
    unwrapped trajectory, a new tensor of the same shape: every atom follows the image nearest to where it was one frame
    before (mdno_unwrap_frames; integer image counts, no accumulated rounding).  A trajectory that never wrapped comes back
    bit for bit."""
    if box is None:
        raise MdnoError("unwrap_frames: box is None: expected three lengths (Lx, Ly, Lz), 0 for an open axis")
    vals = check_box(box, 0.0) or (0.0, 0.0, 0.0)
    shape = tuple(frames.shape) if torch.is_tensor(frames) else None
    frames, S, M, N = _trajectory(frames)
    out = torch.empty((S, M, N, 3), dtype=torch.float32, device=frames.device)
    if S * M * N:
        check(_lib.load().mdno_unwrap_frames(ptr(frames), S, M, N, box_arg(vals), ptr(out), stream_ptr(frames.device)),
              "mdno_unwrap_frames")
    return out.reshape(shape)


# ------------------------------------------------------------------------------------------------
# Ensemble verification (include/mdno_ensemble.h, csrc/ensemble.hip)
ENSEMBLE_SAMPLE_TILE = 256          # MDNO_ENS_SAMPLE_TILE: samples per workgroup (fixes the order of the sums)
MAX_ENSEMBLE_MEMBERS = 1024         # MDNO_ENS_MAX_MEMBERS
MAX_REGISTER_MEMBERS = 64           # MDNO_ENS_MAX_REGISTER_MEMBERS
ENSEMBLE_FORMS = _lib.ENSEMBLE_FORMS


def ensemble_score(frames: torch.Tensor, truth: torch.Tensor, form: str = "auto"):
    """frames f32 [S, M, N, 3] (the M members of one ensemble) against truth f32 [S, N, 3] -> (sums f64 [S, 4],
    rank_hist i64 [S, M + 1], n_invalid i64 [S], n_ties i64 [S]): per step, over its 3 N samples (atom, component), the
    sums of the squared error of the ensemble mean, of the unbiased ensemble variance, of sum_m |x_m - y| and of
    sum_{m<k} |x_m - x_k|, the histogram of the truth's rank among the sorted members, the samples left out because a
    value is not finite (their step's sums are NaN) and the samples where a member equals the truth (include/mdno_ensemble.h
    has the rule; mdnoens_score).  No output depends on the order of the members; fixed summation order: the same bits on
    every run.  `form`: "auto" (registers up to 64 members, LDS up to 1,024), "registers" or "lds" to force one (the same
    bits).  Asynchronous on the current stream, nothing is read back."""
    frames = _device_frames(frames, "frames", (4,))
    truth = _device_frames(truth, "truth", (3,))
    if truth.device != frames.device:
        raise MdnoError(f"truth is on {truth.device}, frames on {frames.device}")
    S, M, N, _ = frames.shape
    if tuple(truth.shape) != (S, N, 3):
        raise MdnoError(f"truth shape {tuple(truth.shape)} does not match frames {tuple(frames.shape)}: expected {(S, N, 3)}")
    code = form_code(form, ENSEMBLE_FORMS)
    if not 1 <= M <= MAX_ENSEMBLE_MEMBERS:
        raise MdnoError(f"ensemble_score: {M} members, expected 1 .. {MAX_ENSEMBLE_MEMBERS}")
    if form == "registers" and M > MAX_REGISTER_MEMBERS:
        raise MdnoError(f"ensemble_score: form 'registers' holds at most {MAX_REGISTER_MEMBERS} members, got {M}")
    check_dims("frames", frames.shape)
    lib = _lib.load()
    dev = frames.device
    sums = torch.empty((S, 4), dtype=torch.float64, device=dev)
    rank_hist = torch.empty((S, M + 1), dtype=torch.int64, device=dev)
    n_invalid = torch.empty((S,), dtype=torch.int64, device=dev)
    n_ties = torch.empty((S,), dtype=torch.int64, device=dev)
    if S == 0:
        return sums, rank_hist, n_invalid, n_ties
    nbytes = lib.mdnoens_score_workspace_bytes(S, M, N)
    ws = _ws(nbytes, dev)
    check(lib.mdnoens_score(ptr(frames) if N else None, ptr(truth) if N else None, S, M, N, ptr(sums), ptr(rank_hist),
                            ptr(n_invalid), ptr(n_ties), code, ptr(ws), nbytes, stream_ptr(dev)),
          "mdnoens_score")
    return sums, rank_hist, n_invalid, n_ties


# ------------------------------------------------------------------------------------------------
# Structural coverage (include/mdno_conformations.h, csrc/conformations.hip)
CONF_FRAME_TILE = 32                # MDNO_CONF_FRAME_TILE: frames per side of a workgroup's tile of pairs
CONF_ATOM_CHUNK = 32                # MDNO_CONF_ATOM_CHUNK: atoms staged per pass (fixes the order of the pair sums)


def cross_rmsd(frames: torch.Tensor, reference: torch.Tensor, matrix: bool = True, nearest: bool = True, cover: bool = True):
    """frames f32 [S, M, N, 3] (or a plain stack [F, N, 3]: M = 1) against reference f32 [Fb, N, 3] -> (matrix f64
    [S, M, Fb], nearest f64 [S, M], nearest_index i64 [S, M], cover f64 [M, Fb], cover_step i64 [M, Fb]), None for what was
    not asked for: the RMSD after the optimal rigid superposition of EVERY frame with EVERY reference frame, per frame the
    smallest of its row and the LOWEST reference index that attains it, per member and reference frame the smallest of the
    member's column and the lowest step that attains it (include/mdno_conformations.h has the rule; mdnoconf_cross_rmsd).
    A frame with a NaN or Inf coordinate gives NaN in its row (column) and is never chosen by an index; NaN and -1 where
    nothing valid is left.  The bits of matrix[s, m, j] depend on the two frames and N alone: fixed summation order, no
    float atomics, the same on every run and inside any batch.  `frames` and `reference` may be the same tensor (the self
    matrix, computed in full).  A periodic `box` is not an argument: a superposition under the minimum image needs whole
    molecules — unwrap first (ops.unwrap_frames) and make them whole.  Asynchronous on the current stream, nothing is read
    back."""
    frames, S, M, N = _trajectory(frames)
    reference = _device_frames(reference, "reference", (3,))
    if reference.device != frames.device:
        raise MdnoError(f"reference is on {reference.device}, frames on {frames.device}")
    Fb = reference.shape[0]
    if reference.shape[1] != N:
        raise MdnoError(f"reference shape {tuple(reference.shape)} does not match frames {tuple(frames.shape)}: expected "
                        f"[Fb, {N}, 3]")
    if not (matrix or nearest or cover):
        raise MdnoError("cross_rmsd: no output was asked for (matrix, nearest and cover are all False)")
    if Fb >= 2 ** 31 * CONF_FRAME_TILE:
        raise MdnoError(f"reference has shape {tuple(reference.shape)}: too many frames for one launch")
    lib = _lib.load()
    dev = frames.device
    f64 = dict(dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    out_m = torch.empty((S, M, Fb), **f64) if matrix else None
    out_n, out_ni = (torch.empty((S, M), **f64), torch.empty((S, M), **i64)) if nearest else (None, None)
    out_c, out_cs = (torch.empty((M, Fb), **f64), torch.empty((M, Fb), **i64)) if cover else (None, None)
    if not any(t is not None and t.numel() for t in (out_m, out_n, out_c)):
        return out_m, out_n, out_ni, out_c, out_cs          # every output asked for is empty: nothing to write
    work = S * M > 0 and Fb > 0
    nbytes = lib.mdnoconf_cross_rmsd_workspace_bytes(S, M, N, Fb, int(cover)) if work else 0
    ws = _ws(nbytes, dev) if work else None
    check(lib.mdnoconf_cross_rmsd(ptr(frames) if work and N else None, S, M, ptr(reference) if work and N else None, Fb, N,
                                  ptr(out_m), ptr(out_n), ptr(out_ni), ptr(out_c), ptr(out_cs), ptr(ws), nbytes,
                                  stream_ptr(dev)), "mdnoconf_cross_rmsd")
    return out_m, out_n, out_ni, out_c, out_cs


# ------------------------------------------------------------------------------------------------
# Essential dynamics (include/mdno_essential.h, csrc/essential.hip)
PCA_TILE = 32                       # MDNO_PCA_TILE: features per side of a workgroup's tile of C
PCA_ROW_PASS = 32                   # MDNO_PCA_ROW_PASS
PCA_ROW_CHUNK = 64                  # MDNO_PCA_ROW_CHUNK: a split's length is a multiple of it
PCA_TARGET_WORKGROUPS = 2048        # MDNO_PCA_TARGET_WORKGROUPS
PCA_MAX_SPLITS = 256                # MDNO_PCA_MAX_SPLITS
PCA_SUM_PARTIALS = 16               # MDNO_PCA_SUM_PARTIALS
PCA_MAX_COMPONENTS = 32             # MDNO_PCA_MAX_COMPONENTS


def covariance_row_split(K: int, D: int, lag: int):
    """(rows per split L, splits) of mdnopca_covariance for K terms of D features: the ROW SPLIT rule of the header."""
    T = -(-D // PCA_TILE)
    tiles = T * (T + 1) // 2 if lag == 0 else T * T
    if K <= 0 or tiles == 0:
        return 0, 0
    want = min(PCA_MAX_SPLITS, max(1, -(-PCA_TARGET_WORKGROUPS // tiles)))
    L = PCA_ROW_CHUNK * -(-K // (want * PCA_ROW_CHUNK))
    return L, -(-K // L)


def _vector_f64(t, what: str, D: int, dev) -> torch.Tensor:
    t = device_tensor(t, what, (1,), dtype=torch.float64)
    if t.shape[0] != D or t.device != dev:
        raise MdnoError(f"{what} has shape {tuple(t.shape)} on {t.device}: expected [{D}] on {dev}")
    return t


def superpose_frames(frames: torch.Tensor, reference: torch.Tensor, aligned: bool = True, rmsd: bool = True):
    """frames f32 [S, M, N, 3] (or a plain stack [F, N, 3]: M = 1) onto reference f32 [N, 3] -> (aligned f32 like frames,
    rmsd f64 [S, M]), None for what was not asked for: every frame after its optimal rigid superposition onto the
    reference — centroid on the reference's centroid, proper rotations only (include/mdno_essential.h has the rule;
    mdnopca_superpose).  A frame with a NaN or Inf coordinate comes back as NaN, with a NaN rmsd.  Fixed summation order:
    the bits of a frame's outputs depend on that frame, the reference and N alone.  Asynchronous on the current stream."""
    frames, S, M, N = _trajectory(frames)
    reference = _device_frames(reference, "reference", (2,))
    if reference.device != frames.device:
        raise MdnoError(f"reference is on {reference.device}, frames on {frames.device}")
    if reference.shape[0] != N:
        raise MdnoError(f"reference shape {tuple(reference.shape)} does not match frames {tuple(frames.shape)}: expected [{N}, 3]")
    if not (aligned or rmsd):
        raise MdnoError("superpose_frames: no output was asked for (aligned and rmsd are both False)")
    lib = _lib.load()
    dev = frames.device
    out_a = torch.empty_like(frames) if aligned else None
    out_r = torch.empty((S, M), dtype=torch.float64, device=dev) if rmsd else None
    if S * M:
        check(lib.mdnopca_superpose(ptr(frames) if N else None, S, M, N, ptr(reference) if N else None, ptr(out_a), ptr(out_r),
                                    stream_ptr(dev)), "mdnopca_superpose")
    return out_a, out_r


def feature_sums(x: torch.Tensor):
    """x f32 [R, D] (device) -> (sum f64 [D], n_invalid i64 [1]): the column sums over the rows in a fixed order and the
    number of rows that hold a NaN or Inf (such a row makes the columns it touches NaN); mdnopca_feature_sums.  The mean
    is sum / R.  Asynchronous on the current stream, nothing is read back."""
    x = device_tensor(x, "x", (2,))
    R, D = x.shape
    check_dims("x", x.shape, (D,))
    lib = _lib.load()
    dev = x.device
    total = torch.empty(D, dtype=torch.float64, device=dev)
    bad = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib.mdnopca_feature_sums(ptr(x) if R * D else None, R, D, ptr(total) if D else None, ptr(bad), stream_ptr(dev)),
          "mdnopca_feature_sums")
    return total, bad


def _features(x, what: str = "x"):
    """(x as contiguous f32 [S, M, D] on the device, S, M, D); [F, D] is M = 1."""
    x = device_tensor(x, what, (2, 3))
    if x.dim() == 2:
        x = x[:, None]
    check_dims(what, x.shape)
    return (x, *x.shape)


def feature_covariance(x: torch.Tensor, mean: torch.Tensor, lag: int = 0) -> torch.Tensor:
    """x f32 [S, M, D] (or [F, D]: M = 1), mean f64 [D], lag >= 0 -> C f64 [D, D], the SUMS
    C[a, b] = sum_m sum_t (x[t, m, a] - mean[a]) (x[t + lag, m, b] - mean[b]) over the M (S - lag) pairs, pooled over the
    members (include/mdno_essential.h has the rule; mdnopca_covariance): one fp64 GEMM on the matrix pipe, the rows
    centred in fp64 on the way in, no fp64 copy of x.  lag 0 is bitwise symmetric; lag >= S gives zeros.  Fixed summation
    order: the same bits on every run.  Asynchronous on the current stream."""
    x, S, M, D = _features(x)
    lag = integer(lag, "lag", 0)
    mean = _vector_f64(mean, "mean", D, x.device)
    lib = _lib.load()
    dev = x.device
    out = torch.empty((D, D), dtype=torch.float64, device=dev)
    if D == 0:
        return out
    work = M * max(S - lag, 0) > 0
    nbytes = lib.mdnopca_covariance_workspace_bytes(S, M, D, lag) if work else 0
    ws = _ws(nbytes, dev) if work else None
    check(lib.mdnopca_covariance(ptr(x) if work else None, S, M, D, ptr(mean), lag, ptr(out), ptr(ws), nbytes, stream_ptr(dev)),
          "mdnopca_covariance")
    return out


def project_features(x: torch.Tensor, mean: torch.Tensor, vectors: torch.Tensor) -> torch.Tensor:
    """x f32 [R, D], mean f64 [D], vectors f64 [D, k] (1 <= k <= PCA_MAX_COMPONENTS) -> P f64 [R, k],
    P[r, c] = sum_a (x[r, a] - mean[a]) vectors[a, c], one running fp64 sum in ascending a (mdnopca_project).
    Asynchronous on the current stream."""
    x = device_tensor(x, "x", (2,))
    R, D = x.shape
    check_dims("x", x.shape, (D,))
    mean = _vector_f64(mean, "mean", D, x.device)
    vectors = device_tensor(vectors, "vectors", (2,), dtype=torch.float64)
    if vectors.shape[0] != D or vectors.device != x.device:
        raise MdnoError(f"vectors has shape {tuple(vectors.shape)} on {vectors.device}: expected [{D}, k] on {x.device}")
    k = vectors.shape[1]
    if not 1 <= k <= PCA_MAX_COMPONENTS:
        raise MdnoError(f"vectors has k = {k} columns: expected 1 .. {PCA_MAX_COMPONENTS}")
    lib = _lib.load()
    dev = x.device
    out = torch.empty((R, k), dtype=torch.float64, device=dev)
    if R:
        check(lib.mdnopca_project(ptr(x) if D else None, R, D, ptr(mean) if D else None, ptr(vectors) if D else None, k, ptr(out),
                                  stream_ptr(dev)), "mdnopca_project")
    return out


# ------------------------------------------------------------------------------------------------
# Markov state models (include/mdno_markov.h, csrc/markov.hip)
MSM_MAX_STATES = 1024               # MDNO_MSM_MAX_STATES
MSM_ROW_TILE = 64                   # MDNO_MSM_ROW_TILE: rows per workgroup of the assignment
MSM_CENTRE_TILE = 64                # MDNO_MSM_CENTRE_TILE: centres per workgroup (the minimum runs over the tiles in order)
MSM_FEATURE_PASS = 32               # MDNO_MSM_FEATURE_PASS
MSM_ARGMAX_TILE = 64                # MDNO_MSM_ARGMAX_TILE: rows per workgroup of the k-centres argmax
MSM_SUM_PARTIALS = 16               # MDNO_MSM_SUM_PARTIALS: partial sums per (state, feature) (fixes the order of the sums)
MSM_SUM_FEATURES = 16               # MDNO_MSM_SUM_FEATURES
MSM_SUM_STATES = 16                 # MDNO_MSM_SUM_STATES
MSM_LDS_STATES = 64                 # MDNO_MSM_LDS_STATES: the largest n_states counted in LDS
MSM_MAX_LAGS = MAX_LAGS             # MDNO_MSM_MAX_LAGS


def _msm_matrix(t, what: str):
    """(`t` as a contiguous device matrix [R, D] of f32 or f64 — anything else is converted to f32 —, its dtype code)."""
    t = device_tensor(t, what, (2,), dtype="float")
    check_dims(what, t.shape, t.shape[1:])
    return t, int(t.dtype == torch.float64)


def _msm_states(k, what: str, low: int = 1) -> int:
    return integer(k, what, low, MSM_MAX_STATES)


def assign_features(x: torch.Tensor, centres: torch.Tensor, origin: Optional[torch.Tensor] = None, labels: bool = True,
                    dist2: bool = True):
    """x [R, D], centres [k, D] (device; both f32 or both f64), origin f64 [D] or None -> (label i32 [R], dist2 f64 [R]),
    None for what was not asked for: the nearest centre of every row and the squared distance to it,
    d2 = max(0, |x - o|^2 + |c - o|^2 - 2 (x - o).(c - o)) in fp64 with the inner products on the fp64 matrix pipe
    (include/mdno_markov.h has the rule; mdnomsm_assign).  The lowest index wins a tie; a row with a NaN or Inf gets -1 and
    NaN, a centre with one is never chosen; k = 0 gives -1 everywhere.  The bits of a row's result depend on that row, the
    centres it is compared with, the origin and D alone.  Asynchronous on the current stream."""
    x, code = _msm_matrix(x, "x")
    centres, ccode = _msm_matrix(centres, "centres")
    R, D = x.shape
    k = centres.shape[0]
    if ccode != code:
        raise MdnoError(f"centres are {centres.dtype}, x is {x.dtype}: expected one element type")
    if centres.shape[1] != D or centres.device != x.device:
        raise MdnoError(f"centres have shape {tuple(centres.shape)} on {centres.device}: expected [k, {D}] on {x.device}")
    if k > MSM_MAX_STATES:
        raise MdnoError(f"centres has k = {k} rows: expected 0 .. {MSM_MAX_STATES}")
    if origin is not None:
        origin = _vector_f64(origin, "origin", D, x.device)
    if not (labels or dist2):
        raise MdnoError("assign_features: no output was asked for (labels and dist2 are both False)")
    lib = _lib.load()
    dev = x.device
    out_l = torch.empty(R, dtype=torch.int32, device=dev) if labels else None
    out_d = torch.empty(R, dtype=torch.float64, device=dev) if dist2 else None
    if R == 0:
        return out_l, out_d
    nbytes = lib.mdnomsm_assign_workspace_bytes(R, k, D)
    ws = _ws(nbytes, dev) if nbytes else None
    check(lib.mdnomsm_assign(ptr(x) if D else None, R, D, code, ptr(centres) if k * D else None, k,
                             ptr(origin) if origin is not None and D else None, ptr(out_l), ptr(out_d), ptr(ws), nbytes,
                             stream_ptr(dev)), "mdnomsm_assign")
    return out_l, out_d


def kcenters(x: torch.Tensor, k: int, first: int = 0):
    """x [R, D] (device, f32 or f64) -> (index i64 [k], radius f64 [k]): deterministic farthest-point seeding from row `first`
    — centre i is the row farthest from the centres before it (the lowest row on a tie, rows with a NaN or Inf never),
    radius[i] the covering radius before it was added, radius[0] = +inf (include/mdno_markov.h has the rule;
    mdnomsm_kcenters).  All k rounds are enqueued on the current stream; nothing is read back."""
    x, code = _msm_matrix(x, "x")
    R, D = x.shape
    k = _msm_states(k, "kcenters: k")
    if k > R:
        raise MdnoError(f"kcenters: k = {k} centres of {R} rows")
    first = integer(first, "kcenters: first", 0, R - 1)
    lib = _lib.load()
    dev = x.device
    index = torch.empty(k, dtype=torch.int64, device=dev)
    radius = torch.empty(k, dtype=torch.float64, device=dev)
    nbytes = lib.mdnomsm_kcenters_workspace_bytes(R, D)
    ws = _ws(nbytes, dev)
    check(lib.mdnomsm_kcenters(ptr(x) if D else None, R, D, code, k, first, ptr(index), ptr(radius), ptr(ws), nbytes,
                               stream_ptr(dev)), "mdnomsm_kcenters")
    return index, radius


def centroid_sums(x: torch.Tensor, label: torch.Tensor, k: int):
    """x [R, D] (device, f32 or f64), label i32 [R], k -> (sums f64 [k, D], counts i64 [k]): per state the sum of its rows
    in a fixed order and their number; labels outside 0 .. k - 1 are skipped, an empty state is zeros
    (mdnomsm_centroid_sums).  Asynchronous on the current stream."""
    x, code = _msm_matrix(x, "x")
    R, D = x.shape
    k = _msm_states(k, "centroid_sums: k")
    label = operand(label, "label", torch.int32, (R,), x.device)
    lib = _lib.load()
    dev = x.device
    sums = torch.empty((k, D), dtype=torch.float64, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    check(lib.mdnomsm_centroid_sums(ptr(x) if R * D else None, R, D, code, ptr(label) if R else None, k, ptr(sums) if D else None,
                                    ptr(counts), stream_ptr(dev)), "mdnomsm_centroid_sums")
    return sums, counts


def check_msm_lags(lags, what: str = "transition_counts"):
    """`lags` as a list of Python ints: 1 .. MAX_LAGS integers >= 1, or MdnoError.  Host only."""
    return int_list(lags, what, "lag", (1, MSM_MAX_LAGS), 1, INT_MAX)


def transition_counts(label: torch.Tensor, n_states: int, lags, pooled: bool = False):
    """label i32 [S, M] (device; [S] is one member), lags -> (counts i64 [L, M or 1, n, n], n_skipped i64 [L]): per lag and
    member (or pooled over the members) the number of origins t with label[t] = from and label[t + lag] = to, sliding
    window; a pair with a label outside 0 .. n - 1 is counted in n_skipped instead (mdnomsm_transition_counts).  Integer
    counts: exact.  Asynchronous on the current stream."""
    label = device_tensor(label, "label", (1, 2), dtype=None)
    if label.dtype != torch.int32:
        raise MdnoError(f"label is {label.dtype} {tuple(label.shape)}: expected int32 [S, M]")
    if label.dim() == 1:
        label = label[:, None]
    S, M = label.shape
    if S > INT_MAX or M > 65535:
        raise MdnoError(f"label has shape {tuple(label.shape)}: expected S < 2^31 and M <= 65535")
    n = _msm_states(n_states, "transition_counts: n_states")
    vals = check_msm_lags(lags)
    lib = _lib.load()
    dev = label.device
    Mo = 1 if pooled else M
    counts = torch.empty((len(vals), Mo, n, n), dtype=torch.int64, device=dev)
    skipped = torch.empty(len(vals), dtype=torch.int64, device=dev)
    check(lib.mdnomsm_transition_counts(ptr(label) if S * M else None, S, M, n, _lag_arg(vals), len(vals), int(bool(pooled)),
                                        ptr(counts) if Mo else None, ptr(skipped), stream_ptr(dev)), "mdnomsm_transition_counts")
    return counts, skipped


# ------------------------------------------------------------------------------------------------
# Internal coordinates (include/mdno_internal.h, csrc/internal.hip)
IC_WORKGROUP = 256                  # MDNO_IC_WORKGROUP: threads of a workgroup
IC_LDS_ATOMS = 2048                 # MDNO_IC_LDS_ATOMS: the largest N whose frames are staged in LDS
IC_MAX_GROUP_FRAMES = 16            # MDNO_IC_MAX_GROUP_FRAMES
IC_FEATURE_CHUNK = 8192             # MDNO_IC_FEATURE_CHUNK: index tuples of a frame one workgroup owns
IC_MAX_BINS = 4096                  # MDNO_IC_MAX_BINS
IC_HIST_ROWS = 4096                 # MDNO_IC_HIST_ROWS: rows a workgroup of the column histogram counts
IC_HIST_TABLE = 8192                # MDNO_IC_HIST_TABLE: counters of its LDS table
IC_HIST_COLUMNS = 128               # MDNO_IC_HIST_COLUMNS: columns whose ranges one launch carries
IC_FORMS = _lib.INTERNAL_FORMS


def ic_frames_per_group(n_atoms: int) -> int:
    """MDNO_IC_FRAMES_PER_GROUP(N): the frames one workgroup of mdnoic_features owns."""
    if n_atoms <= 0 or IC_LDS_ATOMS // n_atoms < 1:
        return 1
    return min(IC_LDS_ATOMS // n_atoms, IC_MAX_GROUP_FRAMES)


def _ic_indices(t, width: int, what: str, dev) -> torch.Tensor:
    """An index array as contiguous int32 [n, width] on `dev` (None: no entries)."""
    if t is None:
        return torch.zeros((0, width), dtype=torch.int32, device=dev)
    t = operand(t, what, (torch.int32, torch.int64), (None, width), dev)
    check_dims(what, t.shape)
    return t.to(torch.int32)


def internal_features(frames: torch.Tensor, pairs=None, triples=None, quads=None, box=None, radians: bool = False,
                      dtype=torch.float32, form: str = "auto") -> torch.Tensor:
    """frames f32 [..., N, 3] and device index arrays pairs i32 [P, 2], triples [A, 3], quads [T, 4] (None: none) ->
    out [..., D] of `dtype` (f32 or f64), D = P + A + 2 T: the distances, the cosines of the angles at the middle atom, then
    (cos, sin) of every dihedral (IUPAC sign), in fp64 on the fp32 coordinates by the rule of include/mdno_internal.h
    (mdnoic_features).  `radians`: angles and dihedrals as one column each, D = P + A + T.  `box` = (Lx, Ly, Lz), 0 for an
    open axis: bond vectors by the minimum image (no cutoff is tested).  An index outside 0 .. N - 1 gives NaN and reads
    nothing.  `form`: "auto" (frames staged in LDS up to IC_LDS_ATOMS atoms), "lds" or "global" to force one (the same
    bits).  Asynchronous on the current stream, nothing is read back."""
    code = form_code(form, IC_FORMS)
    if dtype not in (torch.float32, torch.float64):
        raise MdnoError(f"dtype {dtype}: expected torch.float32 or torch.float64")
    box = check_box(box, 0.0)
    frames, lead, F, N = _flat_frames(frames)
    if form == "lds" and N > IC_LDS_ATOMS:
        raise MdnoError(f"form 'lds' holds frames of at most {IC_LDS_ATOMS} atoms, N = {N}")
    dev = frames.device
    pairs, triples, quads = (_ic_indices(t, w, n, dev) for t, w, n in ((pairs, 2, "pairs"), (triples, 3, "triples"), (quads, 4, "quads")))
    P, A, T = pairs.shape[0], triples.shape[0], quads.shape[0]
    D = P + A + (1 if radians else 2) * T
    check_dims("the feature tensor", lead + (D,), (D,))
    lib = _lib.load()
    out = torch.empty(lead + (D,), dtype=dtype, device=dev)
    check(lib.mdnoic_features(ptr(frames) if F * N else None, F, N, ptr(pairs) if P else None, P, ptr(triples) if A else None, A,
                              ptr(quads) if T else None, T, box_arg(box) if box else None, _lib.INTERNAL_RADIANS if radians else 0,
                              _lib.INTERNAL_DTYPES[str(dtype).split(".")[-1]], ptr(out) if F * D else None, code,
                              stream_ptr(dev)), "mdnoic_features")
    return out


ICG_MAX_ITEMS = _lib.INTERNAL_GRAD_MAX_ITEMS    # MDNO_ICG_MAX_ITEMS: an incidence is item * 4 + slot in an int32
ICG_TARGET_GROUPS = 1024            # MDNO_ICG_TARGET_GROUPS
ICG_MIN_THREADS = 64                # MDNO_ICG_MIN_THREADS


def icg_atom_chunk(n_frames: int, n_atoms: int) -> int:
    """The atoms of a frame group one workgroup of mdnoicg_features_bwd owns (include/mdno_internal_grad.h, FORMS AND GRID)."""
    G = ic_frames_per_group(n_atoms)
    groups = -(-n_frames // G)
    C = n_atoms
    while C > 0 and groups * -(-n_atoms // C) < ICG_TARGET_GROUPS and G * C > ICG_MIN_THREADS:
        C = (C + 1) // 2
    return C


def internal_features_bwd(frames: torch.Tensor, g: torch.Tensor, pairs, triples, quads, atom_ptr: torch.Tensor, inc: torch.Tensor,
                          box=None, dtype=torch.float32, form: str = "auto") -> torch.Tensor:
    """The adjoint of `internal_features` in its default mode: frames f32 [..., N, 3], g [..., D] (f32 or f64, the gradient
    with respect to the features, D = P + A + 2 T), the index arrays of the forward and the incidence table atom_ptr i32
    [N + 1], inc i32 [n_inc] (inc[e] = item * 4 + slot, ascending within an atom: forecast.Featurizer.incidence builds it) ->
    grad [..., N, 3] of `dtype` (f32 or f64): per (frame, atom) one fp64 accumulation chain over the atom's incidences, by
    the rule of include/mdno_internal_grad.h (mdnoicg_features_bwd).  An item whose g is exactly zero is skipped; every
    element is written.  `form` as in `internal_features` (the same bits).  Asynchronous on the current stream, nothing is
    read back."""
    code = form_code(form, IC_FORMS)
    if dtype not in (torch.float32, torch.float64):
        raise MdnoError(f"dtype {dtype}: expected torch.float32 or torch.float64")
    box = check_box(box, 0.0)
    frames, lead, F, N = _flat_frames(frames)
    if form == "lds" and N > IC_LDS_ATOMS:
        raise MdnoError(f"form 'lds' holds frames of at most {IC_LDS_ATOMS} atoms, N = {N}")
    dev = frames.device
    pairs, triples, quads = (_ic_indices(t, w, n, dev) for t, w, n in ((pairs, 2, "pairs"), (triples, 3, "triples"), (quads, 4, "quads")))
    P, A, T = pairs.shape[0], triples.shape[0], quads.shape[0]
    D = P + A + 2 * T
    if P + A + T >= ICG_MAX_ITEMS:
        raise MdnoError(f"{P + A + T} index tuples: the incidence table holds fewer than 2^29")
    g = operand(g, "g", (torch.float32, torch.float64), lead + (D,), dev)
    atom_ptr = operand(atom_ptr, "atom_ptr", torch.int32, (N + 1,), dev)
    inc = operand(inc, "inc", torch.int32, (None,), dev)
    n_inc = inc.shape[0]
    lib = _lib.load()
    grad = torch.empty(lead + (N, 3), dtype=dtype, device=dev)
    dtype_code = lambda t: _lib.INTERNAL_DTYPES[str(t).split(".")[-1]]
    check(lib.mdnoicg_features_bwd(ptr(frames) if F * N else None, F, N, ptr(pairs) if P else None, P, ptr(triples) if A else None, A,
                                   ptr(quads) if T else None, T, ptr(atom_ptr), ptr(inc) if n_inc else None, n_inc,
                                   box_arg(box) if box else None, 0, ptr(g) if F * D else None, dtype_code(g.dtype),
                                   ptr(grad) if F * N else None, dtype_code(dtype), code, stream_ptr(dev)), "mdnoicg_features_bwd")
    return grad


def check_column_ranges(lo, hi, n_bins, D: int):
    """(lo, hi as lists of Python floats — one entry: a range shared by all columns, else D —, n_bins as int) for a column
    histogram, or MdnoError: finite, hi > lo, n_bins in 1 .. IC_MAX_BINS.  Host only."""
    n_bins = integer(n_bins, "column_histogram: n_bins", 1, IC_MAX_BINS)
    vals = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = to_list(v)
        try:
            v = [float(e) for e in v] if hasattr(v, "__len__") or hasattr(v, "__iter__") else [float(v)]
        except (TypeError, ValueError):
            raise MdnoError(f"column_histogram: {name}={v!r}: expected a number or {D} numbers") from None
        vals.append(v)
    lo, hi = vals
    if len(lo) != len(hi) or len(lo) not in (1, D):
        raise MdnoError(f"column_histogram: {len(lo)} lower and {len(hi)} upper bounds for {D} columns: expected 1 or {D} of each")
    for a, (l, h) in enumerate(zip(lo, hi)):
        if not (math.isfinite(l) and math.isfinite(h) and h > l and math.isfinite(h - l)):
            raise MdnoError(f"column_histogram: range [{l}, {h}) of column {a} is not finite or is empty")
    return lo, hi, n_bins


def column_histogram(x: torch.Tensor, lo, hi, n_bins: int, groups: int = 1):
    """x [R, D] (device, f32 or f64), lo and hi (a number each, or D numbers: host values) -> (counts i64 [D, n_bins + 2],
    n_nan i64 [D]): per column the histogram of its values over n_bins equal bins of [lo, hi); counts[:, 0] holds the values
    below lo, counts[:, -1] those at or above hi, a NaN is counted in n_nan alone, so counts.sum(1) + n_nan == R
    (include/mdno_internal.h has the rule; mdnoic_column_histogram).  `groups` = G: x is [R, G D], G groups of D columns
    that share the D ranges (the members of a feature tensor [S, M, D]); counts [G D, n_bins + 2], n_nan [G D].  Integer
    counts: exact.  Asynchronous on the current stream."""
    x, code = _msm_matrix(x, "x")
    R, width = x.shape
    if width % integer(groups, "column_histogram: groups", 1, 65535):
        raise MdnoError(f"column_histogram: groups={groups!r} for {width} columns: expected groups of equally many columns")
    D = width // groups
    lo, hi, n_bins = check_column_ranges(lo, hi, n_bins, D)
    lib = _lib.load()
    dev = x.device
    counts = torch.empty((width, n_bins + 2), dtype=torch.int64, device=dev)
    n_nan = torch.empty(width, dtype=torch.int64, device=dev)
    if D == 0:
        return counts, n_nan
    lo_arg, hi_arg = (C.c_double * len(lo))(*lo), (C.c_double * len(hi))(*hi)
    check(lib.mdnoic_column_histogram(ptr(x) if R else None, R, D, groups, code, lo_arg, hi_arg, int(len(lo) == 1),
                                      n_bins, ptr(counts), ptr(n_nan), stream_ptr(dev)), "mdnoic_column_histogram")
    return counts, n_nan


# ------------------------------------------------------------------------------------------------
# Distance-constraint projection (include/mdno_constrain.h, csrc/constrain.hip)
CST_MAX_ATOMS = _lib.CONSTRAIN_MAX_ATOMS                # MDNOCST_MAX_ATOMS
CST_MAX_CONSTRAINTS = _lib.CONSTRAIN_MAX_CONSTRAINTS    # MDNOCST_MAX_CONSTRAINTS
CST_GROUP_ATOMS = 1024                                  # MDNOCST_GROUP_ATOMS
CST_MAX_GROUP_FRAMES = 16                               # MDNOCST_MAX_GROUP_FRAMES


def cst_frames_per_group(n_atoms: int) -> int:
    """MDNOCST_FRAMES_PER_GROUP(N): the frames one workgroup of mdnocst_project owns."""
    if n_atoms <= 0 or CST_GROUP_ATOMS // n_atoms < 1:
        return 1
    return min(CST_GROUP_ATOMS // n_atoms, CST_MAX_GROUP_FRAMES)


def check_constraint_table(pairs, lo, hi, colour_ptr, weights, n_atoms: int, dev):
    """The coloured table of a projection as the C ABI takes it: pairs i32 [C, 2], lo / hi f64 [C], colour_ptr i32
    [n_colours + 1], weights f32 [n_atoms] or None, all contiguous on `dev`; MdnoError otherwise.  Shapes, dtypes and devices
    only: the values were validated on the host when the table was made (forecast.DistanceConstraints)."""
    pairs = operand(pairs, "pairs", torch.int32, (None, 2), dev)
    n_c = int(pairs.shape[0])
    if n_c > CST_MAX_CONSTRAINTS:
        raise MdnoError(f"{n_c} constraints: more than {CST_MAX_CONSTRAINTS}")
    lo, hi = operand(lo, "lo", torch.float64, (n_c,), dev), operand(hi, "hi", torch.float64, (n_c,), dev)
    colour_ptr = operand(colour_ptr, "colour_ptr", torch.int32, (None,), dev)
    if colour_ptr.shape[0] < 1:
        raise MdnoError("colour_ptr is empty: expected int32 [n_colours + 1]")
    return pairs, lo, hi, colour_ptr, operand(weights, "weights", torch.float32, (n_atoms,), dev, optional=True)


def check_projection_args(iterations, tol):
    return integer(iterations, "iterations", 0), real(tol, "tol", positive=False, finite=False)


def project_constraints(frames: torch.Tensor, pairs: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, colour_ptr: torch.Tensor,
                        weights=None, box=None, iterations: int = 8, tol: float = 0.0, out=None):
    """frames f32 [..., N, 3] and a COLOURED constraint table on the same device (pairs i32 [C, 2], lo / hi f64 [C] sorted by
    colour, colour_ptr i32 [n_colours + 1], weights f32 [N] or None) -> (projected f32 [..., N, 3], sweeps i32 [...],
    viol_in f64 [...], viol_out f64 [...]) by the rule of include/mdno_constrain.h (mdnocst_project): up to `iterations`
    sweeps per frame, until its largest |length - band| is at most `tol`.  `out`: where the frames go (`frames` itself for
    an in-place projection; default: a new tensor).  `box` = (Lx, Ly, Lz), 0 for an open axis: bond vectors by the minimum
    image.  N <= CST_MAX_ATOMS.  Asynchronous on the current stream, nothing is read back."""
    iterations, tol = check_projection_args(iterations, tol)
    box = check_box(box, 0.0)
    frames, lead, F, N = _flat_frames(frames)
    if N > CST_MAX_ATOMS:
        raise MdnoError(f"project_constraints: frames of {N} atoms, the kernel holds at most {CST_MAX_ATOMS} (the state of a frame "
                        f"lies in LDS)")
    dev = frames.device
    pairs, lo, hi, colour_ptr, weights = check_constraint_table(pairs, lo, hi, colour_ptr, weights, N, dev)
    n_c, n_colours = int(pairs.shape[0]), int(colour_ptr.shape[0]) - 1
    if out is None:
        out = torch.empty(lead + (N, 3), dtype=torch.float32, device=dev)
    elif operand(out, "out", torch.float32, lead + (N, 3), dev) is not out:          # (a contiguous tensor comes back as itself)
        raise MdnoError(f"out has strides {out.stride()}: expected a contiguous tensor")
    elif out.data_ptr() != frames.data_ptr() and F * N and \
            out.data_ptr() < frames.data_ptr() + frames.numel() * 4 and frames.data_ptr() < out.data_ptr() + out.numel() * 4:
        raise MdnoError("out overlaps frames without being frames")
    lib = _lib.load()
    sweeps = torch.empty(lead, dtype=torch.int32, device=dev)
    viol_in = torch.empty(lead, dtype=torch.float64, device=dev)
    viol_out = torch.empty(lead, dtype=torch.float64, device=dev)
    check(lib.mdnocst_project(ptr(frames) if F * N else None, ptr(out) if F * N else None, F, N, ptr(pairs) if n_c else None,
                              ptr(lo) if n_c else None, ptr(hi) if n_c else None, n_c, ptr(colour_ptr), n_colours,
                              ptr(weights) if weights is not None and N else None, box_arg(box) if box else None, iterations, tol,
                              ptr(sweeps) if F else None, ptr(viol_in) if F else None, ptr(viol_out) if F else None,
                              stream_ptr(dev)), "mdnocst_project")
    return out, sweeps, viol_in, viol_out


# ------------------------------------------------------------------------------------------------
# Contact statistics over time (include/mdno_contacts.h, csrc/contacts.hip)
CM_TILE = _lib.CONTACTS_TILE        # MDNOCM_TILE: atoms per side of a pair tile
CM_MAX_LAGS = _lib.CONTACTS_MAX_LAGS


def check_contact_args(threshold, box=None, block_len=1, what: str = "pair_statistics"):
    """(threshold as float, box as check_box returns it, block_len as int) or MdnoError: threshold finite and > 0, every
    periodic axis of the box >= 2 * threshold, block_len an integer >= 1 (include/mdno_contacts.h).  Host only."""
    cut = real(threshold, f"{what}: threshold")
    block_len = integer(block_len, f"{what}: block_len", 1)
    return cut, check_box(box, cut), block_len


def _contact_frames(frames, what: str):
    frames = _device_frames(frames, "frames", (4,))
    check_dims(f"{what}: frames", frames.shape)
    return (frames, *frames.shape[:3])


def pair_statistics(frames: torch.Tensor, threshold: float = 8.0, box=None, block_len: int = 64, moments: bool = True):
    """frames f32 [S, M, N, 3] -> (count i32, sum_r f64, sum_r2 f64), each [Bk, M, N, N] with Bk = ceil(S / block_len): per
    pair (both triangles and the diagonal) and block of `block_len` consecutive steps, the frames in which the pair is closer
    than `threshold`, the sum of the distance and the sum of its square, each sum one sequential fp64 chain in step order
    (include/mdno_contacts.h has the rule; mdnocm_pair_statistics).  `moments` False: only the counts (the two sums are
    None, and the kernel takes no square root).  `box` = (Lx, Ly, Lz), 0 for an open axis: distances by the minimum image,
    every periodic axis >= 2 * threshold.  Asynchronous on the current stream, nothing is read back."""
    threshold, box, block_len = check_contact_args(threshold, box, block_len)
    frames, S, M, N = _contact_frames(frames, "pair_statistics")
    lib = _lib.load()
    dev = frames.device
    Bk = -(-S // block_len)
    shape = (Bk, M, N, N)
    count = torch.empty(shape, dtype=torch.int32, device=dev)
    sum_r = torch.empty(shape, dtype=torch.float64, device=dev) if moments else None
    sum_r2 = torch.empty(shape, dtype=torch.float64, device=dev) if moments else None
    work = S * M * N > 0
    check(lib.mdnocm_pair_statistics(ptr(frames) if work else None, S, M, N, threshold, box_arg(box) if box else None, block_len,
                                     ptr(count) if work else None, ptr(sum_r) if work and moments else None,
                                     ptr(sum_r2) if work and moments else None, stream_ptr(dev)), "mdnocm_pair_statistics")
    return count, sum_r, sum_r2


def contact_bits(frames: torch.Tensor, pairs: torch.Tensor, cut: torch.Tensor, cut_max: float, box=None):
    """frames f32 [S, M, N, 3], pairs i32 [P, 2] and cut f64 [P] on the same device -> (bits u64-as-int64 [M, P, Wd],
    per_frame i32 [S, M]), Wd = ceil(S / 64): bit s % 64 of word s / 64 says whether pair p of member m is closer than
    min(cut[p], cut_max) at step s, and per_frame counts the listed pairs in contact per frame (include/mdno_contacts.h (b);
    mdnocm_contact_bits).  torch has no unsigned 64-bit arithmetic: the words are handed back as int64 with the same bits.
    An index outside 0 .. N - 1 is never in contact and reads nothing.  `box`: every periodic axis >= 2 * cut_max.
    Asynchronous on the current stream, nothing is read back."""
    cut_max, box, _ = check_contact_args(cut_max, box, 1, "contact_bits")
    frames, S, M, N = _contact_frames(frames, "contact_bits")
    dev = frames.device
    pairs = _ic_indices(pairs, 2, "pairs", dev)
    P = pairs.shape[0]
    cut = operand(cut, "cut", torch.float64, (P,), dev)
    lib = _lib.load()
    Wd = -(-S // 64)
    bits = torch.empty((M, P, Wd), dtype=torch.int64, device=dev)
    work = S * M * P > 0
    per_frame = torch.empty((S, M), dtype=torch.int32, device=dev) if work else torch.zeros((S, M), dtype=torch.int32, device=dev)
    check(lib.mdnocm_contact_bits(ptr(frames) if work and N else None, S, M, N, ptr(pairs) if work else None,
                                  ptr(cut) if work else None, P, cut_max, box_arg(box) if box else None,
                                  ptr(bits) if work else None, ptr(per_frame) if work else None, stream_ptr(dev)),
          "mdnocm_contact_bits")
    return bits, per_frame


def check_contact_lags(lags, S: int, what: str = "contact_correlation"):
    """`lags` as a list of Python ints: at most CM_MAX_LAGS integers in 0 .. S - 1, or MdnoError.  Host only."""
    return int_list(lags, what, "lag", (0, CM_MAX_LAGS), 0, S - 1)


def contact_correlation(bits: torch.Tensor, S: int, lags):
    """bits int64 [M, P, ceil(S / 64)] (ops.contact_bits) and integer lags in 0 .. S - 1 -> (origins, both) i32 [M, P, L]:
    for every member, pair and lag the steps t < S - lag at which the pair is in contact, and those at which it is in
    contact at t and at t + lag (include/mdno_contacts.h (c); mdnocm_contact_correlation).  Integers, exact.  Asynchronous
    on the current stream, nothing is read back."""
    bits = device_tensor(bits, "bits", None, dtype=None)
    S = integer(S, "contact_correlation: S", 0)
    if bits.dtype != torch.int64 or bits.dim() != 3 or bits.shape[2] != -(-S // 64):
        raise MdnoError(f"bits is {bits.dtype} {tuple(bits.shape)}: expected int64 [M, P, {-(-S // 64)}] for S={S}")
    vals = check_contact_lags(lags, S)
    M, P, _ = bits.shape
    L = len(vals)
    lib = _lib.load()
    dev = bits.device
    work = S * M * P * L > 0
    origins = torch.empty((M, P, L), dtype=torch.int32, device=dev)
    both = torch.empty((M, P, L), dtype=torch.int32, device=dev)
    check(lib.mdnocm_contact_correlation(ptr(bits) if work else None, S, M, P, _lag_arg(vals) if L else None, L,
                                         ptr(origins) if work else None, ptr(both) if work else None, stream_ptr(dev)),
          "mdnocm_contact_correlation")
    return origins, both


# ------------------------------------------------------------------------------------------------
# Solvent-accessible surface (include/mdno_surface.h, csrc/surface.hip)
SA_MAX_POINTS = _lib.SURFACE_MAX_POINTS         # MDNOSA_MAX_POINTS
SA_STAGED_ATOMS = _lib.SURFACE_STAGED_ATOMS     # MDNOSA_STAGED_ATOMS: the largest N of the staged form
SA_TILE = _lib.SURFACE_TILE                     # MDNOSA_TILE
SA_CHUNK = _lib.SURFACE_CHUNK                   # MDNOSA_CHUNK


def check_surface_args(reach, box=None, form: str = "auto"):
    """(reach as float, box as check_box returns it, the form's code) or MdnoError: reach finite and > 0, every periodic axis
    of the box >= 2 * reach, form one of FORECAST_FORMS (include/mdno_surface.h).  Host only."""
    reach = real(reach, "exposed_points: reach")
    return reach, check_box(box, reach), form_code(form, FORECAST_FORMS)


def exposed_points(frames: torch.Tensor, R: torch.Tensor, points: torch.Tensor, box=None, reach=None, form: str = "auto") -> torch.Tensor:
    """frames f32 [..., N, 3], R f64 [N] (the EXPANDED radii r_i + probe) and points f64 [P, 3] (the sphere table, P in
    1 .. 1,024) on the same device -> i32 [..., N]: per atom the points of R_i * points that no neighbour's sphere covers, -1
    for an atom with a non-finite coordinate (include/mdno_surface.h has the rule; mdnosa_exposed_points).  `box` =
    (Lx, Ly, Lz), 0 for an open axis: differences by the minimum image, every periodic axis >= 2 * reach.  `reach` is
    2 * max(R); `forecast.Spheres` carries it on the host, and only where it is left None is it read back from R (the one
    synchronisation this call can make).  Otherwise asynchronous on the current stream, nothing is read back.  `form`:
    "auto" (the frame staged in LDS up to 2,048 atoms, 256-atom tiles above), "lds" or "tiled" to force one (the same
    counts)."""
    frames, lead, F, N = _flat_frames(frames)
    check_dims("exposed_points: frames", frames.shape, (F, N))
    dev = frames.device
    R = operand(R, "R", torch.float64, (N,), dev)
    points = operand(points, "points", torch.float64, (None, 3), dev)
    P = integer(points.shape[0], "exposed_points: the number of points", 1, SA_MAX_POINTS)
    if reach is None:
        reach = 2.0 * float(R.max()) if N else 1.0
    reach, box, code = check_surface_args(reach, box, form)
    lib = _lib.load()
    counts = torch.empty(lead + (N,), dtype=torch.int32, device=dev)
    nbytes = lib.mdnosa_workspace_bytes(F, N, P, code)
    ws = _ws(nbytes, dev) if nbytes else None
    work = F * N > 0
    check(lib.mdnosa_exposed_points(ptr(frames) if work else None, F, N, ptr(R) if work else None, ptr(points), P,
                                    box_arg(box) if box else None, reach, ptr(counts) if work else None, code, ptr(ws), nbytes,
                                    stream_ptr(dev)), "mdnosa_exposed_points")
    return counts
