"""The edge-MLP across its chunk seams.  `edge_mlp()` (csrc/edge_mlp.hip) and `edge_mlp_split()` (csrc/edge_mlp_split.hip)
take at most S = 262,144 edge rows per pass; above that capacity the host loops over chunks, each with its own
`e_begin` / `row_begin`, its own offset into the output (W_e rows, or the k-tiled H whose tile index continues across
chunks) and, in SPLIT_F16, one set of activation flag words zeroed once per forward.  Every production-size workload
crosses that seam; here every output is held to fp64 on the host, as a whole tensor (`close` of test_gpu_parity.py)
AND per slice of ownership:

    each chunk [c S, min((c + 1) S, E)), each seam band [c S - 128, c S + 128) clipped to [0, E), the last 128 valid rows
    err(slice) = |got - want|_slice / max(|want|_slice, |want|_tensor / sqrt(n_slices))          gate 1e-5

(the measure and the forward gate of test_gpu_train_moment_ops.py; the floor is for slices that cancel: a condition,
not a tolerance).  A chunk that is written to the wrong rows, computed from another chunk's rows or left out shows in
its own slice at full size instead of diluted in a tensor of half a million rows.

A  W_e target, `ops.edge_mlp` (mdno_edge_mlp_fwd), ker_width 128 x out_dim 128 x ker_in 6, seeded torch.nn.Linear
   weights, attributes randn * 5.  (edge_cap, num_edges) = (S, S) control, (S+1, S+1) a second chunk of one row,
   (S+300, S) second chunk wholly past the count, (S+300, S-1) / (S+300, S+1) the count next to the seam, (S+300, S+263)
   partial last chunk and tile, (2S+130, 2S+93) three chunks; each in f32, split_bf16 and split_f16, the edge source
   alternating so that every mode sees both past the seam: explicit edge_attr under a random permutation of all E rows
   (row p from edge_attr[perm[p]]: rows after the seam read attributes from before it; and the output equals the
   unpermuted output indexed by perm, bit for bit), or (edge_pos, src, dst) over 77 nodes.  Every run inside guard
   bands under both fills (tests/guarded.py): no byte outside a buffer changes, rows >= num_edges of W_e keep the fill
   (include/mdno.h: not computed), and the valid rows have the same bits under both fills (a later chunk that reads
   an earlier chunk's stale h1 / h2 workspace rows into a valid row differs).  The same at ker_width 100 x out_dim 9.
   Kernels.  At a 262,144-row chunk `both_gemms_small` is false, so the few-rows kernels are out:
     f32, k 128      edge_l0_kernel, gemm_tn_mfma_kernel<true>, gemm_tn_mfma_kernel<false>
     f32, k 100      edge_l0_kernel, gemm_tn_generic_kernel<true>, <false>      (any ker_width off the 128 tile)
     split_bf16      edge_l0_split_kernel<., 0>, gemm_split_bf16 kernels writing planes (layer 1) and fp32 (layer 2)
     split_f16       edge_l0_split_kernel<., 1>, the big-tile fp16 GEMMs (launch_split_f16_gemm) to planes and to fp32,
                     then edge_l0_split_fallback_kernel and the two strided bf16 fallback GEMMs, which exit at once
   (`<., .>`: the attribute count 6 is a template argument for either source.)

C  SPLIT_F16's range flag across chunks, shapes of A at edge_cap = num_edges = S + 300: ONE row's attributes times 3e5
   put its h1 above 65,504 (checked in fp64: that row only; everything finite in fp32).  Read from edge_mlp_split():
   the flag words are zeroed once, before the chunk loop, and every launch is in stream order.  With the wild row in
   the second chunk the first chunk's fp16 chain and its (idle) fallback launches have run before layer 0 of the second
   chunk raises F16_ACT_RANGE, so the first chunk keeps its fp16 result: asserted equal to the tame run's bits.  With
   the wild row in the first chunk the flag stays up for the second, which then runs on the bf16 planes too: accuracy
   only.  Either way every tame row meets the gates (the wild row taken out of both sides), the wild row is within
   1e-5 of fp64 relative to its own norm, under both fills (a chunk skipped by both launches would hold the fill).

B  The H target (k-tiled, reachable only through mdno_kernelnn_fwd with the factored conv) and the W_e target through
   the whole forward: KernelNN width 64, ker_width 128, depth 1, seeded reference init with the last edge-MLP layer
   x 0.2; 5 members x 240 atoms uniform in a ball of radius 3.9 A, cutoff 8: every ordered pair (and every self-loop)
   is an edge, 57,600 per member, E = 288,000, member 4 = edges 230,400 .. 288,000 straddles row S (asserted on the
   device's graph); edge_cap = E + 1000.  conv_mode factored / materialized x the three GEMM modes: out and latent
   against fp64 per member and whole; members 0 and 4 (the straddling and last one) alone, in one chunk, equal their
   slices of the batch bit for bit; in split_f16 the fallback counters are all zero (both chunks ran on fp16 planes).
   The fp64 reference never forms W_e (9 GB): per member, with h_e [k] the edge-MLP's last hidden activation,
       S_i = sum over in-edges e = (j -> i) of x_j (x) h_e                     [64, k]
       y_i = relu((sum_{c,k} S_i[c,k] W2[c*64 + o, k] + sum_c (sum_j x_j)[c] b2[c*64 + o]) / deg_i + x_i root + bias)
   once with conv1's root / bias and once with conv2's; checked against the oracle's per-edge forward on a 12-atom
   complete graph (1e-12) every time the reference is built.

Room under the gate, measured on the CPU (python tests/test_gpu_edge_mlp_seams.py): the same reference in torch float32
against fp64 through the same measure, the largest figure over the whole tensor and all slices.  Least room: 41x.

    A  ker_width 128, edge_attr  cap S        2.2e-07      position-derived  cap S        2.3e-07
                                 cap S+1      2.2e-07                        cap S+1      2.3e-07
                                 cap S+300    2.2e-07                        cap S+300    2.2e-07
                                 cap 2S+130   2.2e-07                        cap 2S+130   2.2e-07
       ker_width 100, edge_attr  cap S+300    2.2e-07      position-derived  cap S+300    2.3e-07
       (per capacity: the largest over its (edge_cap, num_edges) cases)
    C  tame rows 2.2e-07 (both placements)   wild row at S+17, own norm 1.9e-07   wild row at 5, own norm 2.4e-07
    B  out 2.7e-07   latent 1.7e-07
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 262144                      # kMaxChunkRows: what chunk_rows_for (csrc/edge_mlp.hip) gives every capacity from S on
GATE = 1e-5                     # FWD_GATE of test_gpu_train_moment_ops.py, REL_L2 of test_gpu_parity.py
BAND = 128
MODES = ("f32", "split_bf16", "split_f16")
R_NODES = 77


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel_s(n):
    """A row count written relative to S."""
    m = 2 if n > S + S // 2 else 1
    return ("2S" if m == 2 else "S") + (f"{n - m * S:+d}" if n != m * S else "")


# ------------------------------------------------------------------------------------------------ the measure
def spans(E, cap=None):
    """name -> [lo, hi) of every slice of ownership with a valid row in it: the chunks of a capacity `cap`, the bands
    around every multiple of S up to it, the last rows."""
    n_chunks = math.ceil(max(cap or E, E) / S)
    out = {f"chunk {c}": (c * S, min((c + 1) * S, E)) for c in range(n_chunks)}
    out.update({f"seam {c}": (max(c * S - BAND, 0), min(c * S + BAND, E)) for c in range(1, n_chunks + 1)})
    out["last rows"] = (max(E - BAND, 0), E)
    return {n: (lo, hi) for n, (lo, hi) in out.items() if hi > lo}


def row_squares(got, want):
    """Per row: |got - want|^2 and |want|^2, in float64."""
    E = want.shape[0]
    d2, w2 = torch.empty(E, dtype=torch.float64), torch.empty(E, dtype=torch.float64)
    for lo in range(0, E, 65536):
        w = want[lo:lo + 65536].double().reshape(min(65536, E - lo), -1)
        g = got[lo:lo + 65536].double().reshape(w.shape)
        d2[lo:lo + 65536] = ((g - w) ** 2).sum(1)
        w2[lo:lo + 65536] = (w * w).sum(1)
    return d2, w2


def slice_errors(d2, w2, where):
    """"whole" and err(slice) of every slice in `where` from the per-row squares."""
    total = float(w2.sum().sqrt())
    errs = {"whole": float(d2.sum().sqrt()) / max(total, 1e-300)}
    floor = total / math.sqrt(len(where))
    for n, (lo, hi) in where.items():
        errs[n] = float(d2[lo:hi].sum().sqrt()) / max(float(w2[lo:hi].sum().sqrt()), floor, 1e-300)
    return errs


def assert_under_gate(errs, name):
    print(name, {n: f"{v:.1e}" for n, v in errs.items()})
    bad = {n: v for n, v in errs.items() if not v < GATE}
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------ A: inputs, reference
@functools.lru_cache(maxsize=None)
def mlp_weights(kw, od):
    """Seeded torch.nn.Linear default init, as test_edge_mlp_mfma_vs_oracle: the oracle's state dict."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        lins = [torch.nn.Linear(6, kw), torch.nn.Linear(kw, kw), torch.nn.Linear(kw, od)]
    sd = {}
    for j, lin in zip((0, 2, 4), lins):
        sd[f"layers.{j}.weight"], sd[f"layers.{j}.bias"] = lin.weight.data.clone(), lin.bias.data.clone()
    return sd


def mlp_reference(ea, sd, dtype=torch.float64):
    from oracle import graph_kernel_oracle as O
    return O.edge_mlp(ea.to(dtype), {n: v.to(dtype) for n, v in sd.items()}, "")


def edge_inputs(cap, source):
    g = torch.Generator().manual_seed(2 * cap + (source == "pos"))
    if source == "pos":
        pos = torch.randn(R_NODES, 3, generator=g) * 5
        src = torch.randint(0, R_NODES, (cap,), generator=g).to(torch.int32)
        dst = torch.randint(0, R_NODES, (cap,), generator=g).to(torch.int32)
        return dict(pos=pos, src=src, dst=dst, ea=torch.cat([pos[src.long()], pos[dst.long()]], dim=1))
    return dict(ea=torch.randn(cap, 6, generator=g) * 5)


@functools.lru_cache(maxsize=2)         # (the cases are ordered by capacity: two sources of one capacity at a time)
def base(cap, source, kw, od):
    """Inputs of all `cap` rows and their fp64 W_e, UNPERMUTED, once for every mode and count; never modified."""
    t = edge_inputs(cap, source)
    t["want"] = mlp_reference(t["ea"], mlp_weights(kw, od))
    return t


def perm_for(ne):
    """A random permutation of all `ne` valid rows."""
    return torch.randperm(ne, generator=torch.Generator().manual_seed(ne)).to(torch.int32)


def _cases_a():
    out = []
    pairs = [(S, S), (S + 1, S + 1), (S + 300, S), (S + 300, S - 1), (S + 300, S + 1), (S + 300, S + 263), (2 * S + 130, 2 * S + 93)]
    for i, (cap, ne) in enumerate(pairs):
        for j, mode in enumerate(MODES):
            out.append(dict(kw=128, od=128, cap=cap, ne=ne, mode=mode, src=("attr", "pos")[(i + j) % 2]))
    # the unsplit generic kernel: the dispatch of any ker_width that is no multiple of 128
    out.append(dict(kw=100, od=9, cap=S + 300, ne=S + 263, mode="f32", src="attr"))
    out.append(dict(kw=100, od=9, cap=S + 300, ne=S, mode="f32", src="pos"))
    return sorted(out, key=lambda c: (c["kw"], c["cap"]))


def case_id(c):
    return f"k{c['kw']}o{c['od']}-cap{rel_s(c['cap'])}-ne{rel_s(c['ne'])}-{c['mode']}-{c['src']}"


def run_edge_mlp(dev, t, c, ea=None, perm=None, G=None):
    """-> (the valid rows of W_e on the host, whether the rows from num_edges on still hold the guard's fill)."""
    from molecular_dynamics_neural_operator_amd import ops
    cap, ne, sd = c["cap"], c["ne"], mlp_weights(c["kw"], c["od"])
    P = (lambda x: G.place(x.to(dev))) if G is not None else (lambda x: x.to(dev))
    w = [P(sd[f"layers.{j}.{n}"]) for j in (0, 2, 4) for n in ("weight", "bias")]
    count = P(torch.full((1,), ne, dtype=torch.int32))
    if c["src"] == "pos":       # src / dst hold exactly the valid entries: a read at num_edges reads the band
        gr = ops.CSRGraph(None, P(t["src"][:ne]), P(t["dst"][:ne]), count, cap, None, None)
        w_e = ops.edge_mlp(w, 6, c["kw"], c["od"], gr, edge_pos=P(t["pos"]), gemm_mode=c["mode"])
    else:
        gr = ops.CSRGraph(None, None, None, count, cap, P(perm) if perm is not None else None, None)
        ea = t["ea"] if ea is None else ea
        w_e = ops.edge_mlp(w, 6, c["kw"], c["od"], gr, edge_attr=P(ea[:ne]), gemm_mode=c["mode"])
    assert tuple(w_e.shape) == (cap, c["od"])
    kept = True
    if G is not None:
        G.verify()
        kept = not bool(w_e[ne:].contiguous().view(torch.uint8).ne(G.fill).any())
    return w_e[:ne].cpu(), kept


def run_both_fills(dev, t, c, name, **kw):
    from guarded import FILLS, Guard
    res = []
    for fill in FILLS:
        with Guard(fill) as G:
            got, kept = run_edge_mlp(dev, t, c, G=G, **kw)
        assert kept, f"{name}: rows from num_edges on were written (fill {fill:#04x})"
        res.append(got)
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32)), \
        f"{name}: valid rows differ between fill 0x00 and fill 0xFF (read memory nothing wrote)"
    return res[0]


@pytest.mark.parametrize("c", _cases_a(), ids=case_id)
def test_w_e_across_chunk_seams(dev, c):
    """W_e of `ops.edge_mlp` at capacities past one chunk against fp64: whole, per chunk, per seam band, last rows;
    guard bands under both fills, rows >= num_edges untouched, the same bits under both fills, row p from
    edge_attr[perm[p]]."""
    from test_gpu_parity import close
    name, ne = case_id(c), c["ne"]
    t = base(c["cap"], c["src"], c["kw"], c["od"])
    perm = perm_for(ne) if c["src"] == "attr" else None
    got = run_both_fills(dev, t, c, name, perm=perm)
    want = t["want"][perm.long()] if perm is not None else t["want"][:ne]
    assert tuple(got.shape) == tuple(want.shape) == (ne, c["od"])
    assert_under_gate(slice_errors(*row_squares(got, want), spans(ne, c["cap"])), name)
    close(got, want, name=name)
    if perm is not None:        # the same rows in the caller's order, then indexed by perm: the same bits
        plain, _ = run_edge_mlp(dev, t, c)
        assert torch.equal(got, plain[perm.long()]), f"{name}: output under perm != unpermuted output indexed by perm"


# ------------------------------------------------------------------------------------------------ C: the range flag
def wild_inputs(wild):
    """Part A's (S + 300)-row explicit attributes with row `wild` times 3e5; its fp64 W_e row; asserts what the case
    is about: h1 above fp16's range in that row only, everything finite in fp32."""
    cap = S + 300
    t = base(cap, "attr", 128, 128)
    sd = mlp_weights(128, 128)
    ea = t["ea"].clone()
    ea[wild] *= 3.0e5
    h1 = torch.relu(ea.double() @ sd["layers.0.weight"].double().T + sd["layers.0.bias"].double()).max(dim=1).values
    assert float(h1[wild]) > 65504.0
    h1[wild] = 0.0
    assert float(h1.max()) < 65504.0
    assert bool(torch.isfinite(mlp_reference(ea[wild:wild + 1], sd, torch.float32)).all())
    return t, ea, mlp_reference(ea[wild:wild + 1], sd)[0]


def wild_errors(got, t, wild, want_row):
    """(slice errors over the tame rows, the wild row's error relative to its own norm)."""
    d2, w2 = row_squares(got, t["want"])
    d2[wild], w2[wild] = 0.0, 0.0
    own = float((got[wild].double() - want_row).norm() / want_row.norm())
    return slice_errors(d2, w2, spans(got.shape[0])), own


@pytest.mark.parametrize("wild", [S + 17, 5], ids=["wild_row_in_chunk_1", "wild_row_in_chunk_0"])
def test_split_f16_range_flag_across_chunks(dev, wild):
    """One row out of fp16 range in one chunk: every row of both chunks stays within the gates of fp64 (no chunk keeps
    fp16 planes that were out of range, none is skipped by both the fp16 and the bf16 launch); a first chunk that
    finished before the flag went up keeps its fp16 bits."""
    from test_gpu_parity import close
    c = dict(kw=128, od=128, cap=S + 300, ne=S + 300, mode="split_f16", src="attr")
    name = f"wild row {rel_s(wild) if wild > S else wild}"
    t, ea, want_row = wild_inputs(wild)
    tame, _ = run_edge_mlp(dev, t, c)
    got = run_both_fills(dev, t, c, name, ea=ea)
    assert bool(torch.isfinite(got).all())
    errs, own = wild_errors(got, t, wild, want_row)
    print(name, "own norm", f"{own:.1e}")
    assert_under_gate(errs, name)
    assert own < GATE, (name, own)
    close(got[:wild], t["want"][:wild], name=name + ", rows before it")
    close(got[wild + 1:], t["want"][wild + 1:], name=name + ", rows after it")
    if wild >= S:
        assert torch.equal(got[:S], tame[:S]), "the first chunk did not keep its fp16 result"


# ------------------------------------------------------------------------------------------------ B: the whole forward
FWD_M, FWD_N, FWD_W, FWD_K, CUTOFF = 5, 240, 3, 128, 8.0


def seeded_state_dict():
    """The reference's seeded init, the last edge-MLP layer x 0.2 (make_model of tests/test_gpu_unroll.py)."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        model = KernelNN(64, FWD_K, 1, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    return {n: v.detach().clone() for n, v in model.state_dict().items()}


def ball_window(n_atoms, seed, W=FWD_W, radius=3.9):
    """[W, n_atoms, 3]: the last frame uniform in a ball (every pair closer than the cutoff), the earlier ones jittered."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_atoms, 3))
    last = v / np.linalg.norm(v, axis=1, keepdims=True) * (radius * rng.random((n_atoms, 1)) ** (1.0 / 3.0))
    win = last[None] + 0.1 * rng.normal(size=(W, n_atoms, 3))
    win[-1] = last
    return torch.from_numpy(win.astype(np.float32))


def complete_csr(n_atoms):
    """(src, dst) of one member's complete graph with self-loops in destination-sorted CSR order, sources ascending."""
    a = torch.arange(n_atoms)
    return a.repeat(n_atoms), a.repeat_interleave(n_atoms)


def member_reference(sd, window, aa, dtype=torch.float64):
    """(out, latent) of one member on its complete graph in the factored form of the module docstring."""
    from oracle import graph_kernel_oracle as O
    c = {n: v.to(dtype) for n, v in sd.items()}
    N, k = window.shape[1], c["conv1.net.layers.0.weight"].shape[0]
    F = torch.nn.functional
    x = F.linear(O.lstm_last_hidden_functional(window.to(dtype), c), c["lstm_fc.weight"], c["lstm_fc.bias"])
    x = torch.relu(F.linear(torch.cat((F.embedding(aa, c["emb.weight"]), x), dim=1), c["fc1.weight"], c["fc1.bias"]))
    src, dst = complete_csr(N)
    pos = window[-1].to(dtype)
    h = torch.relu(F.linear(torch.cat([pos[src], pos[dst]], dim=1), c["conv1.net.layers.0.weight"], c["conv1.net.layers.0.bias"]))
    h = torch.relu(F.linear(h, c["conv1.net.layers.2.weight"], c["conv1.net.layers.2.bias"])).view(N, N, k)   # [dst, src, k]
    w2 = c["conv1.net.layers.4.weight"].view(64, 64, k).permute(0, 2, 1).reshape(64 * k, 64)                  # [(c, k), o]
    b2 = c["conv1.net.layers.4.bias"].view(64, 64)                                                            # [c, o]
    for conv in ("conv1", "conv2"):
        xs = x[src].view(N, N, 64)
        moment = torch.einsum("ijc,ijk->ick", xs, h)
        msg = moment.reshape(N, 64 * k) @ w2 + xs.sum(1) @ b2
        x = torch.relu(msg / N + x @ c[conv + ".root"] + c[conv + ".bias"])
    return F.linear(x, c["fc2.weight"], c["fc2.bias"]), x


def check_factored_reference(sd):
    """member_reference against the oracle's per-edge forward on a 12-atom complete graph."""
    from oracle import graph_kernel_oracle as O
    n = 12
    win, aa = ball_window(n, 99), torch.arange(n) % 20
    src, dst = complete_csr(n)
    sd64 = {k: v.double() for k, v in sd.items()}
    args = (win.double(), aa, torch.stack([src, dst]), torch.cat([win[-1][src], win[-1][dst]], dim=1).double(), 1)
    eye = {"fc2.weight": torch.eye(64, dtype=torch.float64), "fc2.bias": torch.zeros(64, dtype=torch.float64)}
    with torch.no_grad():
        want = O.kernelnn_forward_autograd(sd64, *args), O.kernelnn_forward_autograd({**sd64, **eye}, *args)
    for got, ref in zip(member_reference(sd, win, aa), want):
        assert float((got - ref).norm() / ref.norm()) < 1e-12


@functools.lru_cache(maxsize=None)
def forward_case():
    """Model, windows [W, M, N, 3], amino acids [M * N] and the fp64 (out, latent) of all members; never modified."""
    base.cache_clear()
    sd = seeded_state_dict()
    check_factored_reference(sd)
    frames = torch.stack([ball_window(FWD_N, 100 + m) for m in range(FWD_M)], dim=1)
    aa = torch.randint(0, 20, (FWD_M * FWD_N,), generator=torch.Generator().manual_seed(4))
    refs = [member_reference(sd, frames[:, m], aa[m * FWD_N:(m + 1) * FWD_N]) for m in range(FWD_M)]
    return dict(sd=sd, frames=frames, aa=aa, out=torch.cat([r[0] for r in refs]), latent=torch.cat([r[1] for r in refs]))


def member_spans(M=FWD_M, N=FWD_N):
    return {f"member {m}": (m * N, (m + 1) * N) for m in range(M)}


def run_forward(dev, t, members, gemm_mode, conv_mode, edge_cap, counts=None):
    """The forward of the given members as one batch -> (out, latent, graph)."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    N = FWD_N
    frames = t["frames"][:, members].contiguous().to(dev)
    aa = torch.cat([t["aa"][m * N:(m + 1) * N] for m in members]).to(dev)
    pos = frames[-1].reshape(-1, 3)
    graph = ops.radius_graph(pos, N, CUTOFF, edge_cap=edge_cap)
    pack = ops.ParamPack(t["sd"], 1, dev, gemm_mode=gemm_mode, conv_mode=conv_mode)
    assert int(_lib.load().mdno_resolve_conv_mode(pack.ref, len(members), edge_cap)) == _lib.CONV_MODES[conv_mode]
    out, latent = ops.kernelnn_forward(pack, frames, aa, graph, edge_pos=pos, return_latent=True, fallback_counts=counts)
    assert int(graph.status.item()) == 0
    return out.cpu(), latent.cpu(), graph


@pytest.mark.parametrize("gemm_mode", MODES)
@pytest.mark.parametrize("conv_mode", ["factored", "materialized"])
def test_forward_across_the_chunk_seam(dev, conv_mode, gemm_mode):
    """out and latent of a 5-member batch whose fifth member's edges straddle row S, against fp64 per member; the
    straddling member and member 0 alone equal their slices of the batch bit for bit; split_f16 takes no fallback."""
    from test_gpu_parity import close
    t = forward_case()
    M, N = FWD_M, FWD_N
    E = M * N * N
    cap = E + 1000
    assert E > S + BAND and cap % 256 != 0
    counts = {} if gemm_mode == "split_f16" else None
    out, latent, graph = run_forward(dev, t, list(range(M)), gemm_mode, conv_mode, cap, counts)
    # the graph is the complete one, member after member: row S strictly inside the fifth member's edges
    assert graph.edge_count() == E
    row_ptr = graph.row_ptr.cpu().long()
    assert torch.equal(row_ptr, torch.arange(M * N + 1) * N)
    src, dst = complete_csr(N)
    offs = (torch.arange(M) * N).repeat_interleave(N * N)
    assert torch.equal(graph.src[:E].cpu().long(), src.repeat(M) + offs) and torch.equal(graph.dst[:E].cpu().long(), dst.repeat(M) + offs)
    straddler = 4
    lo, hi = int(row_ptr[straddler * N]), int(row_ptr[(straddler + 1) * N])
    print(f"E {E}, member {straddler} = edges {lo} .. {hi}, seam at {S}")
    assert lo + BAND < S < hi - BAND
    name = f"{conv_mode} {gemm_mode}"
    for what, got in (("latent", latent), ("out", out)):
        assert bool(torch.isfinite(got).all()), what
        assert_under_gate(slice_errors(*row_squares(got, t[what]), member_spans()), f"{name} {what}")
        close(got, t[what], name=f"{name} {what}")
        for m in range(M):
            close(got[m * N:(m + 1) * N], t[what][m * N:(m + 1) * N], name=f"{name} {what} member {m}")
    if counts is not None:
        print(name, counts)
        assert counts and all(v == 0 for v in counts.values()), counts
    for m in sorted({0, straddler, M - 1}):             # alone: own graph, one chunk
        solo_out, solo_latent, g1 = run_forward(dev, t, [m], gemm_mode, conv_mode, N * N + 1000)
        assert g1.edge_count() == N * N < S
        assert torch.equal(solo_latent, latent[m * N:(m + 1) * N]), (name, "latent", m)
        assert torch.equal(solo_out, out[m * N:(m + 1) * N]), (name, "out", m)


# ------------------------------------------------------------------------------------------------ the room (CPU)
def _room():
    """float32 against fp64 through the same measure: the table of the module docstring."""
    def worst(errs):
        return max(errs.values())
    for kw, od, caps in ((128, 128, [(S, [S]), (S + 1, [S + 1]), (S + 300, [S, S - 1, S + 1, S + 263]), (2 * S + 130, [2 * S + 93])]),
                         (100, 9, [(S + 300, [S + 263, S])])):
        for cap, counts in caps:
            for source in ("attr", "pos"):
                t = base(cap, source, kw, od)
                f32 = mlp_reference(t["ea"], mlp_weights(kw, od), torch.float32)
                d2, w2 = row_squares(f32, t["want"])
                fig = max(worst(slice_errors(d2[:ne], w2[:ne], spans(ne, cap))) for ne in counts)
                print(f"A k{kw} {source:4s} cap {rel_s(cap):7s} {fig:.1e}")
    for wild in (S + 17, 5):
        t, ea, want_row = wild_inputs(wild)
        f32 = mlp_reference(ea, mlp_weights(128, 128), torch.float32)
        errs, own = wild_errors(f32, t, wild, want_row)
        print(f"C wild row {wild}: tame rows {worst(errs):.1e}, own norm {own:.1e}")
    t = forward_case()
    refs = [member_reference(t["sd"], t["frames"][:, m], t["aa"][m * FWD_N:(m + 1) * FWD_N], torch.float32) for m in range(FWD_M)]
    for i, what in enumerate(("out", "latent")):
        got = torch.cat([r[i] for r in refs])
        print(f"B {what} {worst(slice_errors(*row_squares(got, t[what]), member_spans())):.1e}")


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    _room()
