"""Every form of the radius graph and of the COO -> CSR sort (csrc/graph.hip, csrc/graph_small.h) at the sizes where one
form hands over to the next, on degenerate frames, and past one pass over the cell list's atom mask.

The forms share one contract: the same edges, destinations ascending, sources ascending inside a row.  The open graph
is compared with tests/graph_ref.py (a sparse fp64 restatement of the pair rule, itself checked against scipy's dense
matrix in tests/test_graph_ref_host.py), the periodic graph with the dense restatement of tests/test_gpu_pbc.py, the
sorts with torch.sort(stable=True) on the CPU.  Every comparison is on integers, or on float bits for the periodic
attribute rows: np.array_equal on row_ptr, src[:E], dst[:E], num_edges and status.  Random frames assert the input
condition of an exact comparison (no pair within 1e-9, relative, of the cutoff); frames that put pairs AT the cutoff
use exactly representable coordinates instead.

Where a case runs inside guard bands (tests/guarded.py) it runs under both fill bytes: the bands must be intact — in
particular nothing is written at index `edge_cap` — and the valid extents must have the same bits under both fills,
which is also the run-to-run comparison (the atomic slot and scatter orders differ between runs)."""
import numpy as np
import pytest
import torch

import graph_ref as ref
from guarded import FILLS, Guard

pytestmark = pytest.mark.gpu

OVERFLOW = 1            # MDNO_STATUS_EDGE_OVERFLOW (asserted against _lib below)


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    assert _lib.STATUS_EDGE_OVERFLOW == OVERFLOW
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(x):
    """A device or host tensor as a numpy array; floats as their bit patterns."""
    x = x.detach().cpu().contiguous()
    return (x.view(torch.int32) if x.dtype == torch.float32 else x).numpy().copy()


def valid(g, attr=None):
    """The valid extents of a device graph (and of its attribute rows)."""
    e = int(g.num_edges.item())
    out = dict(row_ptr=g.row_ptr, src=g.src[:e], dst=g.dst[:e], num_edges=g.num_edges, status=g.status)
    if attr is not None:
        out["attr"] = attr[:e]
    return out


def expected(want, cap, attr=False):
    """What a builder must leave for the reference graph `want` under edge capacity `cap`: the prefix, row_ptr clipped
    at the capacity, the overflow bit iff an edge was dropped."""
    E = int(want["src"].size)
    e = min(E, cap)
    out = dict(row_ptr=np.minimum(want["row_ptr"], cap).astype(np.int32), src=want["src"][:e], dst=want["dst"][:e],
               num_edges=np.array([e], np.int32), status=np.array([OVERFLOW if E > cap else 0], np.int32))
    if attr:
        out["attr"] = np.ascontiguousarray(want["attr"][:e], dtype=np.float32).view(np.int32)
    return out


def assert_same(got, exp, what):
    for k, v in exp.items():
        a = got[k] if isinstance(got[k], np.ndarray) else bits(got[k])
        assert a.dtype == v.dtype and np.array_equal(a, v), f"{what}: {k} differs"


def both_fills(run):
    """run(G) -> {name: {field: tensor}} of valid extents.  Under each fill byte: the bands of every allocation intact
    after the run; then the same bits under both fills.  Returns the first result as numpy arrays.  (Not
    test_gpu_bounds.both_fills: that one records the entry points it sees into the table its own last test checks.)"""
    res = []
    for fill in FILLS:
        with Guard(fill, record_calls=False) as G:
            out = run(G)
            G.verify()
            res.append({n: {k: bits(v) for k, v in d.items()} for n, d in out.items()})
    assert res[0].keys() == res[1].keys()
    for n in res[0]:
        for k in res[0][n]:
            assert np.array_equal(res[0][n][k], res[1][n][k]), f"{n}.{k} differs between fill 0x00 and fill 0xFF"
    return res[0]


def still_fill(x, G):
    """Nothing wrote this part of an allocation made under guard G."""
    return x.numel() == 0 or bool((x.contiguous().view(torch.uint8) == G.fill).all())


# ============================================================================== a. form boundaries of the open graph
CUT = 8.0
FORM_SHAPES = [
    # one workgroup (R <= 128 and N <= 128): the jb halves at 64 atoms, both scan waves, the last row
    (1, 63, {}), (1, 64, {}), (1, 65, {}), (1, 127, {}), (1, 128, {}), (2, 64, {}), (4, 32, {}), (128, 1, {}),
    # just outside it
    (1, 129, {}), (3, 43, {}), (129, 1, {}), (2, 65, {}),
    # brute force: 64-lane tails of a row, 4-rows-per-block tails
    (1, 192, {}), (1, 193, {}), (5, 51, {}),
    # scan_chunk's carry on and next to a 1,024-row chunk edge
    (1, 1023, {}), (1, 1024, {}), (1, 1025, {}), (2, 1024, {}), (1, 2049, {}), (2049, 1, {}),
    # kCellMinAtoms: the last brute-force size, the first cell-list size in both forms
    (1, 8191, {}), (1, 8192, dict(cell_list=True)), (1, 8192, dict(cell_list=False)),
]


def form_frames(M, N):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    return np.stack([syn.box_frame(N, seed=1000 + 31 * N + 7 * M + m) for m in range(M)]).astype(np.float32).reshape(M * N, 3)


@pytest.mark.parametrize("M,N,kw", FORM_SHAPES, ids=[f"{M}x{N}" + ("" if not kw else "-cell" if kw["cell_list"] else "-brute")
                                                    for M, N, kw in FORM_SHAPES])
def test_open_graph_at_form_boundaries(dev, M, N, kw):
    """edge_cap exactly E, E - 1 (the prefix, flagged) and the minimum R, inside guard bands."""
    from molecular_dynamics_neural_operator_amd import ops
    pos = form_frames(M, N)
    want = ref.radius_graph_members(pos, N, CUT)
    ref.check_condition(want)
    E, R = int(want["src"].size), M * N
    assert E >= R
    caps = dict(tight=E, short=max(E - 1, R), rows=R)

    def run(G):
        p = G.place(t(pos, dev))
        out = {}
        for tag, cap in caps.items():
            g = ops.radius_graph(p, N, CUT, edge_cap=cap, **kw)
            assert g.src.numel() == cap and g.dst.numel() == cap
            out[tag] = valid(g)
        return out

    got = both_fills(run)
    print(f"M={M} N={N} {kw}: E={E} ({E / R:.1f} per atom), margin {want['margin']:.1e}")
    for tag, cap in caps.items():
        assert_same(got[tag], expected(want, cap), f"M={M} N={N} {kw} cap={tag}")
    assert int(got["tight"]["status"][0]) == 0
    assert bool(int(got["short"]["status"][0]) & OVERFLOW) == (E - 1 >= R)


# ============================================================================== b. the cell list against the reference
def cell_cases():
    """The slab (one cell across two axes), the cloud wider than 32 cells per axis and the lattice with pairs exactly at
    the cutoff, built as test_gpu_parity.test_radius_graph_cell_list_equals_brute_force builds them."""
    rng = np.random.default_rng(5)
    slab = (rng.random((1, 12000, 3)) * np.array([400.0, 6.0, 5.0])).astype(np.float32)
    rng.random((1, 8200, 3))                                        # (that test's "one cell" case: the complete graph)
    cloud = (rng.random((1, 20000, 3)) * 900.0).astype(np.float32)
    grid = np.stack(np.meshgrid(np.arange(21), np.arange(21), np.arange(21), indexing="ij"), -1).reshape(1, -1, 3).astype(np.float32) * 2.0
    return {"slab": (slab[0], 8.0, True), "wide cloud": (cloud[0], 10.0, True), "lattice at the cutoff": (grid[0], 4.0, False)}


@pytest.mark.parametrize("name", ["slab", "wide cloud", "lattice at the cutoff"])
def test_cell_list_equals_the_reference(dev, name):
    from molecular_dynamics_neural_operator_amd import ops
    pos, cut, random_coordinates = cell_cases()[name]
    N = pos.shape[0]
    want = ref.radius_graph(pos, cut)
    if random_coordinates:
        ref.check_condition(want)
    else:
        assert want["margin"] == 0.0                                 # pairs AT the cutoff: proposed, refused by the strict <
    cap = N * 700
    assert N >= 8192 and N <= want["src"].size <= cap
    x = t(pos, dev)
    print(f"{name}: N={N} E={want['src'].size} margin {want['margin']:.1e}")
    for cell_list in (True, False):
        assert_same(valid(ops.radius_graph(x, N, cut, edge_cap=cap, cell_list=cell_list)), expected(want, cap),
                    f"{name} cell_list={cell_list}")


def test_cell_list_two_mask_windows(dev):
    """One member of 65,728 atoms: the cell list passes twice over its 65,536-bit mask (w0 = 65,536 in the second
    pass), 2,580 rows read sources out of both passes.  Cell list and brute force equal the reference; a second cell-list
    run has the same bits; a capacity that ends inside the rows of the second window gives the prefix, flagged."""
    from molecular_dynamics_neural_operator_amd import ops
    pos, want = ref.two_window_reference()
    N = pos.shape[0]
    assert N == 65728 and want["src"].size == ref.TWO_WINDOW_EDGES
    ref.check_condition(want)
    assert ref.rows_in_both_windows(want, 65536)[0] >= 1000
    cap = 64 * N
    x = t(pos, dev)
    first = valid(ops.radius_graph(x, N, ref.TWO_WINDOW_CUTOFF, edge_cap=cap, cell_list=True))
    assert_same(first, expected(want, cap), "two windows, cell list")
    assert_same(valid(ops.radius_graph(x, N, ref.TWO_WINDOW_CUTOFF, edge_cap=cap, cell_list=False)), expected(want, cap),
                "two windows, brute force")
    again = valid(ops.radius_graph(x, N, ref.TWO_WINDOW_CUTOFF, edge_cap=cap, cell_list=True))
    assert all(np.array_equal(bits(first[k]), bits(again[k])) for k in first)
    short = int(want["row_ptr"][65600])
    assert N <= short < want["src"].size
    assert_same(valid(ops.radius_graph(x, N, ref.TWO_WINDOW_CUTOFF, edge_cap=short, cell_list=True)), expected(want, short),
                "two windows, cell list, capacity = row_ptr[65600]")


def test_cell_list_two_mask_windows_inside_guard_bands(dev):
    from molecular_dynamics_neural_operator_amd import ops
    pos, want = ref.two_window_reference()
    N, E = pos.shape[0], int(want["src"].size)

    def run(G):
        p = G.place(t(pos, dev))
        return dict(tight=valid(ops.radius_graph(p, N, ref.TWO_WINDOW_CUTOFF, edge_cap=E, cell_list=True)),
                    short=valid(ops.radius_graph(p, N, ref.TWO_WINDOW_CUTOFF, edge_cap=E - 1, cell_list=True)))

    got = both_fills(run)
    assert_same(got["tight"], expected(want, E), "two windows under guard, cap = E")
    assert_same(got["short"], expected(want, E - 1), "two windows under guard, cap = E - 1")


# ============================================================================== c. degenerate frames, all four forms
PBC_CUT = 4.0
FORMS = {"one_workgroup": 40, "brute_force": 300, "cell_list": 8200, "periodic": 130}


def base_frame(form):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    N = FORMS[form]
    if form == "periodic":
        from test_gpu_pbc import BOXES, random_frame
        return random_frame(N, BOXES["three_lengths"], seed=21), PBC_CUT, BOXES["three_lengths"]
    return syn.box_frame(N, seed=300 + N).astype(np.float32), CUT, None


def reference_of(pos, cutoff, box):
    """(graph, has attribute rows): graph_ref for the open forms, the dense periodic restatement under a box."""
    if box is None:
        want = ref.radius_graph(pos, cutoff)
        if cutoff > 0.0:
            ref.check_condition(want)
        return want, False
    return ref.pbc_graph_degenerate(pos, cutoff, box), True


def run_form(dev, G, pos, N, cutoff, box, cap):
    """One graph of one member through the form its size and box select, inside guard G -> (graph, attr or None)."""
    from molecular_dynamics_neural_operator_amd import ops
    p = G.place(t(pos, dev))
    if box is None:
        return ops.radius_graph(p, N, cutoff, edge_cap=cap), None
    return ops.radius_graph_pbc(p, N, cutoff, box, edge_cap=cap)


def degenerate_case(dev, pos, cutoff, box, what):
    N = pos.shape[0]
    want, has_attr = reference_of(pos, cutoff, box)
    cap = max(int(want["src"].size), N)

    def run(G):
        g, attr = run_form(dev, G, pos, N, cutoff, box, cap)
        return dict(g=valid(g, attr))

    got = both_fills(run)
    assert_same(got["g"], expected(want, cap, attr=has_attr), what)
    return want, got["g"]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_nonfinite_atoms_are_in_no_pair(dev, form):
    """5 atoms with a NaN coordinate, 3 with +Inf, 2 with -Inf (atoms 0 and N - 1 among them): empty rows, in no other
    row, no self-loop; every other row is the reference's.  The frames a diverged rollout hands to the builders."""
    base, cutoff, box = base_frame(form)
    pos, bad = ref.with_nonfinite(base, seed=5)
    want, got = degenerate_case(dev, pos, cutoff, box, f"{form}, non-finite atoms")
    assert np.all(np.diff(got["row_ptr"])[bad] == 0) and not np.isin(got["src"], bad).any()
    assert got["src"].size >= pos.shape[0] - 10 and want["src"].size > 2 * pos.shape[0]
    # NaN atoms alone (no infinite bounding box: the cell grid keeps its cells)
    only_nan = np.where(np.isinf(pos), np.float32(np.nan), pos)
    degenerate_case(dev, only_nan, cutoff, box, f"{form}, NaN atoms only")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_coincident_atoms_are_edges_both_ways(dev, form):
    base, cutoff, box = base_frame(form)
    pos, pairs = ref.with_copies(base, seed=6)
    want, got = degenerate_case(dev, pos, cutoff, box, f"{form}, coincident atoms")
    have = set(zip(got["dst"].tolist(), got["src"].tolist()))
    assert all((a, b) in have and (b, a) in have for a, b in pairs.tolist())


@pytest.mark.parametrize("form", sorted(FORMS))
def test_cutoff_zero_gives_no_edge(dev, form):
    """E = 0: row_ptr all zero, count 0, status 0; src holds the staged in-degrees in [0, R) and nothing else is written —
    src past R, dst and the attribute rows keep the fill they were allocated with, and the bands are intact."""
    base, _, box = base_frame(form)
    pos, _ = ref.with_copies(base, seed=7)                           # distance 0 < 0 is false as well
    N = pos.shape[0]
    want, has_attr = reference_of(pos, 0.0, box)
    assert want["src"].size == 0 and not want["row_ptr"].any()
    for cap in (N, N + 64):
        def run(G):
            g, attr = run_form(dev, G, pos, N, 0.0, box, cap)
            torch.cuda.synchronize()
            assert g.src.numel() == cap and still_fill(g.src[N:], G) and still_fill(g.dst, G)
            assert (attr is not None) == has_attr and (attr is None or (attr.shape == (cap, 6) and still_fill(attr, G)))
            return dict(g=valid(g, attr))
        got = both_fills(run)
        assert_same(got["g"], expected(want, cap, attr=has_attr), f"{form}, cutoff 0, cap {cap}")
        assert not got["g"]["row_ptr"].any() and int(got["g"]["num_edges"][0]) == 0 and int(got["g"]["status"][0]) == 0


# ============================================================================== d. the periodic form past one scan chunk
@pytest.mark.parametrize("box", ["cubic", "open_axis"])
@pytest.mark.parametrize("M,N", [(1, 1025), (9, 128)])
def test_periodic_graph_past_the_first_scan_chunk(dev, M, N, box):
    """R = 1,025 and 1,152 rows: attribute rows written from row_ptr values that carry over a 1,024-row chunk edge."""
    from test_gpu_pbc import BOXES, random_frame
    from molecular_dynamics_neural_operator_amd import ops
    L = BOXES[box]
    pos = np.concatenate([random_frame(N, L, seed=5000 + 10 * N + m + len(box)) for m in range(M)])
    want = ref.pbc_graph_members(pos, N, PBC_CUT, L)                 # (asserts the input condition per member)
    E = int(want["src"].size)
    x = t(pos, dev)
    print(f"M={M} N={N} {box}: E={E} ({E / (M * N):.1f} per atom)")
    for cap in (E, E - 1):
        g, attr = ops.radius_graph_pbc(x, N, PBC_CUT, L, edge_cap=cap)
        assert_same(valid(g, attr), expected(want, cap, attr=True), f"periodic M={M} N={N} {box} cap={cap}")
        g, attr = ops.radius_graph_pbc(x, N, PBC_CUT, L, edge_cap=cap, with_attr=False)
        assert attr is None
        assert_same(valid(g), expected(want, cap), f"periodic M={M} N={N} {box} cap={cap}, topology only")


# ============================================================================== e. COO -> CSR and by-source
BIG = 2048              # kBigRow: a row of BIG entries takes the per-wave rank sort, BIG + 1 a workgroup


def sort_cases():
    """name -> (num_nodes, edge_index i64 [2, E])."""
    g = torch.Generator().manual_seed(2049)
    ri = lambda lo, hi, n: torch.randint(lo, hi, (n,), generator=g)
    shuffled = lambda ei: ei[:, torch.randperm(ei.shape[1], generator=g)]
    out = {}
    for E in (2047, 2048, 2049, 3072, 4096, 4097):                   # one row holds all of E (3,072 / 4,096: no partial tile)
        out[f"one row, E={E}"] = (3, torch.stack([ri(0, 3, E), torch.ones(E, dtype=torch.long)]))
    for E in (2048, 2049):                                           # E on either side of the big-row launch, no big row
        out[f"spread, E={E}"] = (64, torch.stack([ri(0, 64, E), ri(0, 64, E)]))
    tgt = torch.cat([torch.full((BIG,), 1), torch.full((BIG + 1,), 2), torch.full((7,), 0), torch.full((5,), 4)])
    out["rows of 2048 and 2049, then an empty row"] = (5, shuffled(torch.stack([ri(0, 5, tgt.numel()), tgt])))
    for hub in (2048, 2049, 5000):                                   # a hub SOURCE: the big row of the by-source sort
        src = torch.cat([torch.full((hub,), 7), ri(8, 200, 3000)])
        out[f"hub source, {hub} out-edges"] = (200, shuffled(torch.stack([src, ri(0, 200, src.numel())])))
    for n in (1, 3, 4, 5, 1023, 1024, 1025):                         # 4-rows-per-block tails, the 1,024-row scan edge
        lo, hi = (0, 1) if n == 1 else (1, n - 1)                    # (n >= 3: nodes 0 and n - 1 have no in-edge)
        out[f"{n} nodes"] = (n, torch.stack([ri(0, n, 3000), ri(lo, hi, 3000)]))
    ei = torch.stack([ri(0, 50, 20000), torch.sort(ri(0, 50, 20000)).values])
    ei[1, :3000] = 0                                                 # (a big row as well)
    out["ids shuffled"] = (50, shuffled(ei))
    return out


SORT_CASES = sort_cases()


@pytest.mark.parametrize("name", list(SORT_CASES))
def test_coo_to_csr_and_by_source_at_row_boundaries(dev, name):
    """Both sorts against torch.sort(stable=True), under both fills (two runs: the atomic slot order differs, the
    result may not)."""
    from molecular_dynamics_neural_operator_amd import ops
    n, ei = SORT_CASES[name]
    E = ei.shape[1]

    def run(G):
        g = ops.coo_to_csr(G.place(ei.to(dev)), n)
        s = ops.source_sorted(g, n)
        return dict(by_dst=dict(row_ptr=g.row_ptr, src=g.src[:E], dst=g.dst[:E], perm=g.perm[:E], num_edges=g.num_edges,
                                status=g.status),
                    by_src=dict(row_ptr=s.row_ptr, nbr=s.src[:E], rowid=s.dst[:E], perm=s.perm[:E], status=s.status))

    got = both_fills(run)
    i32 = lambda x: x.to(torch.int32).numpy()
    ptr = lambda keys: i32(torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(keys, minlength=n).cumsum(0)]))
    order = torch.sort(ei[1], stable=True).indices
    s_src, s_dst = ei[0][order], ei[1][order]
    assert_same(got["by_dst"], dict(row_ptr=ptr(ei[1]), src=i32(s_src), dst=i32(s_dst), perm=i32(order),
                                    num_edges=np.array([E], np.int32), status=np.zeros(1, np.int32)), name)
    order2 = torch.sort(s_src, stable=True).indices
    assert_same(got["by_src"], dict(row_ptr=ptr(ei[0]), nbr=i32(s_dst[order2]), rowid=i32(s_src[order2]), perm=i32(order2),
                                    status=np.zeros(1, np.int32)), name + ", by source")
    deg = np.diff(got["by_dst"]["row_ptr"])
    print(f"{name}: E={E}, largest row {deg.max()} by destination, {np.diff(got['by_src']['row_ptr']).max()} by source")
    if name == "ids shuffled":                                       # the input is far from CSR order: the ids move
        assert int((ei[1][1:] < ei[1][:-1]).sum()) > E // 4 and int((order != torch.arange(E)).sum()) > E // 2
