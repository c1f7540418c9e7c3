"""The gradient of the internal coordinates on the device (include/mdno_internal_grad.h; csrc/internal_grad.hip) against the
numpy restatement (tests/internal_grad_ref.py: the header's fp64 operations in the header's order, the atom's incidences in
the table's order), which tests/test_internal_grad_host.py holds to fp64 autograd.

Gate: BIT-EQUAL to the restatement in f64 grad, bit-equal to its value rounded once in f32 grad, for g in f32 and in f64, in
both forms and between them — the rule uses + - x / sqrt rint only, each correctly rounded, in a fixed order, without
contraction, and the sum is one chain per (frame, atom).  (A NaN equals a NaN: the sign and payload of an invalid operation's
result are not the rule's.)  Shapes are sized from the header's constants (workgroup 256, IC_LDS_ATOMS, IC_FRAMES_PER_GROUP,
the atom chunk); none is the workload's own."""
import numpy as np
import pytest
import torch

import internal_grad_ref as gref
import internal_ref as ref

pytestmark = pytest.mark.gpu

WG, LDS_ATOMS, GROUP_MAX = 256, 2048, 16


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def on(dev, x):
    return torch.from_numpy(np.array(x, order="C")).to(dev)                # (a copy: the shared inputs are read-only)


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit-equal, a NaN matching any NaN."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    view = np.int64 if got.dtype == np.float64 else np.int32
    return bool(np.all((got.view(view) == want.view(view)) | (np.isnan(got) & np.isnan(want))))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def tuples(rng, n, width, N):
    """n index tuples of distinct atoms (where N allows it)."""
    if n == 0:
        return np.zeros((0, width), np.int32)
    if N < width:
        return rng.integers(0, N, size=(n, width)).astype(np.int32)
    first = rng.integers(0, N, size=(n, 1))
    steps = np.stack([rng.choice(np.arange(1, N), size=width - 1, replace=False) for _ in range(n)]) if N <= 64 else \
        np.cumsum(rng.integers(1, (N - 1) // (width - 1) + 1, size=(n, width - 1)), 1)
    return np.concatenate([first, (first + steps) % N], 1).astype(np.int32)


def case(N, F, P, A, T, seed):
    rng = np.random.default_rng(seed)
    frames = (rng.normal(size=(F, N, 3)) * 3.0).astype(np.float32)
    g = rng.normal(size=(F, P + A + 2 * T))
    return frames, g, tuples(rng, P, 2, N), tuples(rng, A, 3, N), tuples(rng, T, 4, N)


def forms_of(N):
    return ("lds", "global") if N <= LDS_ATOMS else ("global",)


def table_of(pairs, triples, quads, N):
    ptr, inc = gref.incidence(pairs.tolist(), triples.tolist(), quads.tolist(), N)
    return ptr.astype(np.int32), inc.astype(np.int32)


def run(dev, frames, g, pairs, triples, quads, table=None, **kw):
    from molecular_dynamics_neural_operator_amd import ops
    ptr, inc = table_of(pairs, triples, quads, frames.shape[1]) if table is None else table
    dp, dt, dq = (on(dev, a) if a is not None and len(a) else None for a in (pairs, triples, quads))
    return ops.internal_features_bwd(on(dev, frames), on(dev, g), dp, dt, dq, on(dev, ptr), on(dev, inc), **kw)


def check_case(dev, frames, g, pairs, triples, quads, box=None):
    """Both forms, g and grad in both types, against the restatement; returns the f64 result (f64 g) of the automatic form."""
    N = frames.shape[1]
    args = (pairs.tolist(), triples.tolist(), quads.tolist(), box)
    table = table_of(pairs, triples, quads, N)
    g32 = g.astype(np.float32)
    wants = {torch.float64: gref.features_bwd(frames, g, *args)[0], torch.float32: gref.features_bwd(frames, g32, *args)[0]}
    outs = []
    for form in forms_of(N) + ("auto",):
        for g_arr, g_type in ((g, torch.float64), (g32, torch.float32)):
            want = wants[g_type]
            with np.errstate(over="ignore"):
                want32 = want.astype(np.float32)
            got = run(dev, frames, g_arr, pairs, triples, quads, table, box=box, dtype=torch.float64, form=form)
            got32 = run(dev, frames, g_arr, pairs, triples, quads, table, box=box, dtype=torch.float32, form=form)
            assert got.shape == want.shape == got32.shape and got.dtype == torch.float64 and got32.dtype == torch.float32
            a, a32 = got.cpu().numpy(), got32.cpu().numpy()
            bad = np.argwhere(~((a.view(np.int64) == want.view(np.int64)) | (np.isnan(a) & np.isnan(want))))
            assert same_bits(a, want), (form, g_type, len(bad), bad[:4].tolist(), [(a[tuple(b)], want[tuple(b)]) for b in bad[:4]])
            assert same_bits(a32, want32), (form, g_type)
            if g_type == torch.float64:
                outs.append(got)
    assert all(same(outs[0], o) for o in outs[1:])
    return outs[-1]


def test_header_constants():
    from molecular_dynamics_neural_operator_amd import ops
    assert (ops.IC_WORKGROUP, ops.IC_LDS_ATOMS, ops.IC_MAX_GROUP_FRAMES) == (WG, LDS_ATOMS, GROUP_MAX)
    assert ops.ic_frames_per_group(128) == 16 and ops.ic_frames_per_group(129) == 15 and ops.ic_frames_per_group(LDS_ATOMS + 1) == 1
    assert ops.icg_atom_chunk(3, 28) == 4 and ops.icg_atom_chunk(3, 2048) == 64 and ops.icg_atom_chunk(3, 2049) == 33


# ================================================================================================ 1. the rule, bit for bit
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 28, 63, 64, 65, 128, 129, 504, LDS_ATOMS, LDS_ATOMS + 1])
def test_gradient_equals_the_restatement_at_every_size(dev, N):
    """All three kinds, 180 items (the restatement walks them one by one), three frames: several atom chunks at every N > 4,
    more than one frame group from N = 1025 on.  128 -> 129 is where a group drops from 16 frames to 15."""
    frames, g, pairs, triples, quads = case(N, 3, 70, 60, 50, seed=N)
    out = check_case(dev, frames, g, pairs, triples, quads)
    assert out.shape == (3, N, 3)
    if N >= 28:
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.1


@pytest.mark.parametrize("N,F", [(28, 1), (28, GROUP_MAX - 1), (28, GROUP_MAX), (28, GROUP_MAX + 1), (28, 3 * GROUP_MAX + 2),
                                 (129, 14), (129, 15), (129, 16), (129, 47)])
def test_gradient_equals_the_restatement_at_every_frame_count(dev, N, F):
    """F in {1, G - 1, G, G + 1, 3 G + 2} for G = 16 (N = 28) and G = 15 (N = 129)."""
    from molecular_dynamics_neural_operator_amd import ops
    G = ops.ic_frames_per_group(N)
    assert F in (1, G - 1, G, G + 1, 3 * G + 2)
    frames, g, pairs, triples, quads = case(N, F, 40, 30, 30, seed=100 + F)
    assert check_case(dev, frames, g, pairs, triples, quads).shape == (F, N, 3)


@pytest.mark.parametrize("empty", ["pairs", "triples", "quads", "all"])
def test_gradient_with_an_empty_kind(dev, empty):
    n = lambda kind: 0 if empty in (kind, "all") else 33
    frames, g, pairs, triples, quads = case(65, GROUP_MAX + 1, n("pairs"), n("triples"), n("quads"), seed=200)
    out = check_case(dev, frames, g, pairs, triples, quads)
    if empty == "all":                                                                  # D == 0: zeros, every element written
        assert g.shape[1] == 0 and not bool(out.view(torch.int64).any())


# ================================================================================================ 2. hubs and duplicates
def test_a_hub_duplicates_and_indices_outside_the_frame(dev):
    N, F, hub, lone = 65, GROUP_MAX + 1, 7, 64
    frames, g, pairs, triples, quads = case(N - 1, F, 30, 30, 30, seed=300)              # (tuples among atoms 0 .. 63)
    frames = np.concatenate([frames, np.full((F, 1, 3), 2.5, np.float32)], 1)            # atom 64 is in no item
    spokes = np.array([(hub, j % (N - 1)) if j % 2 else (j % (N - 1), hub) for j in range(310)], np.int32)     # (7, 7) among them
    pairs = np.concatenate([pairs, spokes, [(3, 3)], pairs[:2], [(-1, 5)], [(5, N)]]).astype(np.int32)
    triples = np.concatenate([triples, [(9, 11, 9)], triples[4:5], [(1, N, 2)]]).astype(np.int32)
    quads = np.concatenate([quads, quads[:1], [(2 ** 31 - 1, 1, 2, 3)], [(5, 5, 6, 7)]]).astype(np.int32)
    g = np.random.default_rng(301).normal(size=(F, len(pairs) + len(triples) + 2 * len(quads)))
    g[:, -2:] = 0.0                                                                      # the quad (5, 5, 6, 7) is degenerate: masked out
    ptr, inc = table_of(pairs, triples, quads, N)
    assert ptr[hub + 1] - ptr[hub] > 300 and ptr[lone + 1] == ptr[lone]
    out = check_case(dev, frames, g, pairs, triples, quads).cpu().numpy()
    assert np.isfinite(out).all()
    assert not out[:, lone].view(np.int64).any()                                         # +0.0, written
    # the items with an index outside the frame contribute nothing: dropping them changes no bit
    keep = run(dev, frames, np.delete(g, [len(pairs) - 2, len(pairs) - 1, len(pairs) + len(triples) - 1,
                                          len(pairs) + len(triples) + 2 * (len(quads) - 2), len(pairs) + len(triples) + 2 * (len(quads) - 2) + 1], 1),
               pairs[:-2], triples[:-1], np.delete(quads, len(quads) - 2, 0), dtype=torch.float64)
    assert same_bits(keep.cpu().numpy(), out)


# ================================================================================================ 3. degenerate and non-finite
def test_degenerate_geometry_and_non_finite_values(dev):
    N, F = 28, GROUP_MAX + 1
    frames, g, pairs, triples, quads = case(N, F, 40, 40, 40, seed=400)
    for t in range(2, len(quads)):                                                       # quad 0 alone holds its j, k, l, put on a line below
        if set(quads[0][1:].tolist()) <= set(quads[t].tolist()):
            quads[t] = quads[t - 1]
    assert not set(quads[0][1:].tolist()) <= set(quads[1].tolist())
    base = check_case(dev, frames, g, pairs, triples, quads).cpu().numpy()
    assert np.isfinite(base).all()
    P, A = len(pairs), len(triples)
    # j, k, l of quad 0 on a line (n2 = 0 exactly): NaN for its four atoms with g != 0; with its g zeroed, the gradient of
    # the same items without that quad
    i, j, k, l = quads[0]
    step = np.array([0.5, 1.25, -0.75], np.float32)
    line = frames.copy()
    line[:, j] = (1.0, -2.0, 0.5)
    line[:, k], line[:, l] = line[:, j] + step, line[:, j] + 2 * step
    assert np.isnan(ref.features(line, quads=quads[:1].tolist())).all()
    out = check_case(dev, line, g, pairs, triples, quads).cpu().numpy()
    assert np.isnan(out[:, [i, j, k, l]]).any(axis=-1).all()
    masked = g.copy()
    masked[:, P + A:P + A + 2] = (0.0, -0.0)
    out = check_case(dev, line, masked, pairs, triples, quads).cpu().numpy()
    assert np.isfinite(out).all()
    without = run(dev, line, np.delete(masked, [P + A, P + A + 1], 1), pairs, triples, quads[1:], dtype=torch.float64)
    assert same_bits(without.cpu().numpy(), out)
    # a NaN coordinate: exactly the atoms that share a non-skipped item with it, in that frame
    for frame, atom in ((2, 13), (GROUP_MAX, 0)):
        bad = frames.copy()
        bad[frame, atom, 1] = np.nan
        gz = g.copy()
        first = next(t for t in range(P) if atom in pairs[t])
        gz[:, first] = 0.0                                                               # one of its pairs is skipped: it carries nothing
        out = check_case(dev, bad, gz, pairs, triples, quads).cpu().numpy()
        want_clean = gref.features_bwd(frames, gz, pairs.tolist(), triples.tolist(), quads.tolist())[0]
        hit = {atom}
        for t, tup in enumerate(list(pairs) + list(triples) + list(quads)):
            if atom in tup and t != first:
                hit |= set(int(a) for a in tup)
        only_by_first = set(int(a) for a in pairs[first]) - hit
        rows = np.arange(F) != frame
        assert same_bits(out[rows], want_clean[rows])
        hit = sorted(hit)
        clean = [a for a in range(N) if a not in hit]
        assert np.isnan(out[frame, hit]).all() and len(clean) > 0 and same_bits(out[frame, clean], want_clean[frame, clean])
        assert all(a in clean for a in only_by_first)
    # a NaN in g: the atoms of that item, in that frame
    gn = g.copy()
    gn[1, P + 3] = np.nan
    out = check_case(dev, frames, gn, pairs, triples, quads).cpu().numpy()
    members = sorted(set(int(a) for a in triples[3]))
    others = [a for a in range(N) if a not in members]
    assert np.isnan(out[1, members]).all() and same_bits(out[1, others], base[1, others]) and same_bits(out[[0, 2]], base[[0, 2]])


# ================================================================================================ 4. periodic boxes
@pytest.mark.parametrize("box", [(9.0, 9.0, 9.0), (9.0, 0.0, 7.5)])
def test_gradient_under_a_box(dev, box):
    rng = np.random.default_rng(int(sum(box) * 4))
    N, F = 65, 3
    L = np.array([l if l > 0 else 9.0 for l in box])
    frames = (rng.random(size=(F, N, 3)) * L).astype(np.float32)
    near = rng.random(size=(F, N, 3)) < 0.3                                            # atoms a hair inside opposite faces
    frames = np.where(near, np.where(rng.random(size=(F, N, 3)) < 0.5, np.float32(1e-3), (L - 1e-3).astype(np.float32)), frames).astype(np.float32)
    _, g, pairs, triples, quads = case(N, F, 60, 50, 40, seed=17)
    out = check_case(dev, frames, g, pairs, triples, quads, box=box)
    free = check_case(dev, frames, g, pairs, triples, quads, box=None)
    assert not same(out, free)                                                         # (the box did something)
    crossing = sum(1 for i, j in pairs if np.abs(frames[:, j].astype(np.float64) - frames[:, i]).max() > L.min() / 2)
    assert crossing > 5                                                                # bonds across the boundary
    assert same(run(dev, frames, g, pairs, triples, quads, box=(0.0, 0.0, 0.0), dtype=torch.float64), free)


# ================================================================================================ 5. independence
def test_a_gradient_row_depends_on_its_frame_alone(dev):
    N, F = 28, 2 * GROUP_MAX + 3
    frames, g, pairs, triples, quads = case(N, F, 50, 40, 40, seed=500)
    full = run(dev, frames, g, pairs, triples, quads, dtype=torch.float64)
    assert same(run(dev, frames, g, pairs, triples, quads, dtype=torch.float64), full)                  # two runs
    assert same(run(dev, frames, g, pairs, triples, quads, dtype=torch.float64, form="global"), full)   # the forms
    for f in (0, GROUP_MAX - 1, GROUP_MAX, F - 1):                                                       # alone or inside a batch
        for form in ("lds", "global"):
            assert same(run(dev, frames[f:f + 1], g[f:f + 1], pairs, triples, quads, dtype=torch.float64, form=form), full[f:f + 1])
    # [S, M, N, 3] with g [S, M, D] is the flat stack, reshaped
    from molecular_dynamics_neural_operator_amd import ops
    ptr, inc = table_of(pairs, triples, quads, N)
    sm = ops.internal_features_bwd(on(dev, frames[:32]).reshape(16, 2, N, 3), on(dev, g[:32]).reshape(16, 2, -1), on(dev, pairs),
                                   on(dev, triples), on(dev, quads), on(dev, ptr), on(dev, inc), dtype=torch.float64)
    assert sm.shape == (16, 2, N, 3) and same(sm.reshape(32, N, 3), full[:32])


# ================================================================================================ 6. a table that lies
def _corrupt_table(pairs, triples, quads, N):
    ptr, inc = table_of(pairs, triples, quads, N)
    ptr, inc = ptr.copy(), inc.copy()
    items = len(pairs) + len(triples) + len(quads)
    lo = int(ptr[0])
    assert ptr[1] - ptr[0] >= 4
    inc[lo] = 4 * items                                                                # an item out of range
    inc[lo + 1] = -3                                                                   # a negative entry
    inc[lo + 2] = inc[int(ptr[5])]                                                     # a slot that names another atom
    inc[lo + 3] = (inc[lo + 3] & ~3) | 3 if inc[lo + 3] < 4 * len(pairs) else inc[lo + 3]   # slot 3 of a pair
    ptr[3] = -7                                                                        # atom 2 ends, atom 3 starts, before the table
    ptr[N] = len(inc) + 100000                                                         # the last atom's range runs past it
    ptr[N // 2] = 2 ** 31 - 1                                                          # and one in the middle, both ways
    return ptr, inc


def _run_guarded(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    res = []
    with Guard(fill, record_calls=False) as G:
        for N, F, form in ((28, GROUP_MAX + 1, "lds"), (65, 3, "global"), (LDS_ATOMS, 2, "lds"), (LDS_ATOMS + 1, 2, "auto")):
            frames, g, pairs, triples, quads = case(N, F, 60, 50, 40, seed=600 + N)
            pairs[:8, 0] = 0                                                            # atom 0 has entries to corrupt
            pairs[9], quads[1] = (-1, N), (0, 1, 2, N)                                   # out-of-range indices read nothing
            ptr, inc = _corrupt_table(pairs, triples, quads, N)
            args = [G.place(on(dev, a)) for a in (frames, g.astype(np.float32), pairs, triples, quads, ptr, inc)]
            for dtype in (torch.float32, torch.float64):
                res.append(ops.internal_features_bwd(*args, box=(9.0, 0.0, 7.0), dtype=dtype, form=form).clone())
            want = gref.features_bwd(frames, g.astype(np.float32), pairs.tolist(), triples.tolist(), quads.tolist(), (9.0, 0.0, 7.0),
                                     table=(ptr, inc))[0]
            res.append(want)
        G.verify()
    return res


def test_a_corrupt_table_stays_inside_the_buffers(dev):
    """Every input and the output inside guard bands under both fill bytes (tests/guarded.py), with a table whose items,
    slots and ranges lie: every band intact, every element of grad written (identical under 0x00 and 0xFF, no NaN from the
    0xFF fill), the entries that are right still counted (the restatement walks the same table)."""
    from guarded import FILLS
    a, b = (_run_guarded(dev, fill) for fill in FILLS)
    assert len(a) == len(b) == 4 * 3
    for i in range(0, len(a), 3):
        for u, v in zip(a[i:i + 2], b[i:i + 2]):
            assert same(u, v) and bool(torch.isfinite(u).all()), i
        assert same_bits(a[i + 1].cpu().numpy(), a[i + 2]) and float(np.abs(a[i + 2]).max()) > 0.1
        with np.errstate(over="ignore"):
            assert same_bits(a[i].cpu().numpy(), a[i + 2].astype(np.float32))


# ================================================================================================ 7. autograd
def test_internal_coordinates_is_differentiable(dev):
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    N, F = 28, GROUP_MAX + 1
    ft = forecast.Featurizer.backbone(N)
    rng = np.random.default_rng(700)
    frames = np.cumsum(rng.normal(size=(F, N, 3)) * 2.0, 1).astype(np.float32)
    args = (ft.pairs.tolist(), ft.triples.tolist(), ft.quads.tolist())
    for dtype, np_type in ((torch.float32, np.float32), (torch.float64, np.float64)):
        g = rng.normal(size=(F, ft.dim())).astype(np_type)
        x = on(dev, frames).requires_grad_()
        out = forecast.internal_coordinates(x, ft, dtype=dtype)
        assert out.grad_fn is not None and out.requires_grad
        assert same(out, ops.internal_features(on(dev, frames), *(t.to(dev) for t in (ft.pairs, ft.triples, ft.quads)), dtype=dtype))
        out.backward(on(dev, g))
        with np.errstate(over="ignore"):
            want = gref.features_bwd(frames, g, *args)[0].astype(np.float32)
        assert x.grad.dtype == torch.float32 and same_bits(x.grad.cpu().numpy(), want)
    assert (N, str(dev)) in ft._incidence and len(ft._incidence) == 1                    # built once, on the caller's instance
    # sum().backward() hands over a stride-0 g; [S, M, N, 3]; a box
    x = on(dev, frames[:16]).reshape(8, 2, N, 3).requires_grad_()
    forecast.internal_coordinates(x, ft, box=(30.0, 0.0, 25.0)).sum().backward()
    want = gref.features_bwd(frames[:16], np.ones((16, ft.dim()), np.float32), *args, box=(30.0, 0.0, 25.0))[0].astype(np.float32)
    assert same_bits(x.grad.cpu().numpy().reshape(16, N, 3), want)
    # f64 frames are read as their f32 value (as the forward reads them) and get an f64 gradient
    x = on(dev, frames.astype(np.float64)).requires_grad_()
    forecast.internal_coordinates(x, ft, dtype=torch.float64).sum().backward()
    assert x.grad.dtype == torch.float64
    assert same_bits(x.grad.cpu().numpy(), gref.features_bwd(frames, np.ones((F, ft.dim())), *args)[0])
    # radians has no gradient
    with pytest.raises(MdnoError, match="not differentiable"):
        forecast.internal_coordinates(on(dev, frames).requires_grad_(), ft, radians=True)
    assert forecast.internal_coordinates(on(dev, frames).requires_grad_().detach(), ft, radians=True).shape == (F, ft.dim(True))


def test_without_requires_grad_nothing_changes(dev, monkeypatch):
    """The same single library call, the same bits; so under no_grad with frames that require grad."""
    from molecular_dynamics_neural_operator_amd import _lib, forecast, ops
    lib = _lib.load()
    called = []
    for name in list(_lib.INTERNAL_SIGNATURES) + list(_lib.INTERNAL_GRAD_SIGNATURES):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (called.append(name), real(*a))[1])(real, name))
    N = 28
    ft = forecast.Featurizer.backbone(N).to(dev)
    frames = on(dev, case(N, 5, 0, 0, 0, seed=800)[0])
    want = ops.internal_features(frames, ft.pairs, ft.triples, ft.quads)
    called.clear()
    out = forecast.internal_coordinates(frames, ft)
    assert called == ["mdnoic_features"] and out.grad_fn is None and same(out, want)
    called.clear()
    with torch.no_grad():
        out = forecast.internal_coordinates(frames.clone().requires_grad_(), ft)
    assert called == ["mdnoic_features"] and out.grad_fn is None and same(out, want)
    called.clear()
    x = frames.clone().requires_grad_()
    forecast.internal_coordinates(x, ft).sum().backward()
    assert called == ["mdnoic_features", "mdnoicg_features_bwd"]


# ================================================================================================ 8. StructureLoss
def test_structure_loss_gradient_equals_the_restatement(dev, monkeypatch):
    """B = 3, N = 28, a base without a gradient: d loss / d out is the kernel's result for the f32 g that torch's mean, square
    and difference hand it — bit-equal to the restatement fed that g."""
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd.training import StructureLoss
    B, N = 3, 28
    ft = forecast.Featurizer.backbone(N, 3, 4)
    rng = np.random.default_rng(900)
    y = np.cumsum(rng.normal(size=(B, N, 3)) * 2.0, 1).astype(np.float32)
    out = (y + rng.normal(size=y.shape) * 0.3).astype(np.float32)
    seen = []
    real = ops.internal_features_bwd
    monkeypatch.setattr(ops, "internal_features_bwd", lambda frames, g, *a, **kw: (seen.append(g.clone()), real(frames, g, *a, **kw))[1])
    loss_fn = StructureLoss(lambda o, t: o.new_zeros(()), ft, weight=(1.0, 0.5, 2.0))
    o = on(dev, out.reshape(B, -1)).requires_grad_()
    loss = loss_fn(o, on(dev, y.reshape(B, -1)))
    loss.backward()
    assert len(seen) == 1 and seen[0].dtype == torch.float32 and seen[0].shape == (B, ft.dim())
    g = seen[0].cpu().numpy()
    assert np.isfinite(g).all() and (g != 0).all()
    with np.errstate(over="ignore"):
        want = gref.features_bwd(out, g, ft.pairs.tolist(), ft.triples.tolist(), ft.quads.tolist())[0].astype(np.float32)
    assert same_bits(o.grad.cpu().numpy().reshape(B, N, 3), want)
    # the value: the three means, weighted, to f32 rounding of a few hundred terms
    f_o, f_y = (ref.features(a, ft.pairs.tolist(), ft.triples.tolist(), ft.quads.tolist()) for a in (out, y))
    P, A = ft.pairs.shape[0], ft.triples.shape[0]
    d2 = (f_o - f_y) ** 2
    value = 1.0 * d2[:, :P].mean() + 0.5 * d2[:, P:P + A].mean() + 2.0 * d2[:, P + A:].mean()
    assert abs(float(loss.detach()) - value) <= 1e-4 * value
    l2, mse = loss_fn.rel_with_mse(o.detach(), on(dev, y.reshape(B, -1)))
    assert float(l2) == float(loss.detach()) and abs(float(mse) - float(((out - y) ** 2).mean())) < 1e-6


@pytest.mark.parametrize("unroll", [1, 2])
def test_structure_loss_of_weight_zero_is_the_base(dev, unroll):
    """The smallest model configuration of tests/test_gpu_unroll.py (ker_width 128, depth 1, N = 28, four members): every
    parameter gradient bit for bit as with the base alone."""
    from test_gpu_unroll import make_model, small_trajectory
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import StructureLoss, _unrolled_loss, train_forward
    dtraj = small_trajectory(dev)
    base = LpLoss(size_average=False)
    grads = []
    for loss_fn in (base, StructureLoss(base, forecast.Featurizer.backbone(28), weight=0.0)):
        model = make_model(128, 1, dev)
        batch = dtraj.batch(range(0, 4), unroll=unroll) if unroll > 1 else dtraj.batch(range(0, 4))
        if unroll > 1:
            l2, _ = _unrolled_loss(model, batch, 4, unroll, loss_fn, 8.0, False)
        else:
            out = train_forward(model, batch)
            l2, _ = loss_fn.rel_with_mse(out.view(4, -1), batch.y.view(4, -1))
        l2.backward()
        grads.append((float(l2), {n: p_.grad.clone() for n, p_ in model.named_parameters()}))
    assert grads[0][0] == grads[1][0] and len(grads[0][1]) > 10
    for n, v in grads[0][1].items():
        assert torch.equal(v, grads[1][1][n]) and bool(torch.isfinite(v).all()), n
    assert any(float(v.abs().max()) > 0 for v in grads[0][1].values())


def test_structure_loss_trains(dev):
    """train_epoch over two batches with weight = 1: finite losses, above the base's, and parameters that moved."""
    from test_gpu_unroll import make_model, small_trajectory
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, StructureLoss, train_epoch, validate_epoch
    dtraj = small_trajectory(dev)
    base = LpLoss(size_average=False)
    loss_fn = StructureLoss(base, forecast.Featurizer.backbone(28, 3, 4), weight=1.0)
    model = make_model(128, 1, dev)
    before = {n: p_.detach().clone() for n, p_ in model.named_parameters()}
    base_loss, base_mse = validate_epoch(model, [dtraj.batch(range(s, s + 4)) for s in (0, 4)], base)
    val_loss, val_mse = validate_epoch(model, [dtraj.batch(range(s, s + 4)) for s in (0, 4)], loss_fn)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    loss, mse = train_epoch(model, [dtraj.batch(range(s, s + 4)) for s in (0, 4)], opt, loss_fn)
    assert all(np.isfinite(v) for v in (loss, mse, val_loss, val_mse)) and val_loss > base_loss and val_mse == base_mse
    moved = [n for n, p_ in model.named_parameters() if not torch.equal(p_.detach(), before[n])]
    assert len(moved) > 10 and all(bool(torch.isfinite(p_).all()) for p_ in model.parameters())
    loss2, _ = train_epoch(model, [dtraj.batch(range(s, s + 4), unroll=2) for s in (0, 4)], opt, loss_fn, unroll=2)
    assert np.isfinite(loss2)


def test_structure_loss_under_the_data_parallel_trainer(dev):
    """DataParallelTrainer takes the loss as it is (an LpLoss with its base's reduction); at world size 1 its pass over two
    batches is train_epoch's, bit for bit."""
    from test_gpu_unroll import make_model, small_trajectory
    from molecular_dynamics_neural_operator_amd import forecast
    from molecular_dynamics_neural_operator_amd.data_parallel import DataParallelTrainer
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    from molecular_dynamics_neural_operator_amd.training import Adam, StructureLoss, train_epoch
    dtraj = small_trajectory(dev)
    runs = []
    for parallel in (False, True):
        loss_fn = StructureLoss(LpLoss(size_average=False), forecast.Featurizer.backbone(28, 3, 4), weight=(1.0, 0.5, 0.5))
        model = make_model(128, 1, dev)
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
        if parallel:
            res = DataParallelTrainer(model, opt, loss_fn).train_epoch([list(range(s, s + 4)) for s in (0, 4)], source=dtraj)
        else:
            res = train_epoch(model, [dtraj.batch(range(s, s + 4)) for s in (0, 4)], opt, loss_fn)
        runs.append((res, {n: p_.detach().clone() for n, p_ in model.named_parameters()}))
    assert runs[0][0] == runs[1][0] and all(np.isfinite(v) for v in runs[0][0])
    for n, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][n]), n
