"""Structural coverage without a GPU: what is particular to include/mdno_conformations.h and its ctypes table (that
header, table and exports agree is tests/test_cabi_tables.py's); every refusal of the header comes back before any device work; the workspace size
is monotone; the arithmetic of forecast.CrossRmsd holds on closed-form toys; and the two routes of the numpy restatement
(tests/cross_rmsd_ref.py: Horn's eigenvalue, explicit Kabsch) agree inside the gate the GPU tests use."""
import re

import numpy as np
import pytest
import torch

import cross_rmsd_ref as ref
from cabi import CSRC, INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_conformations.h"
NAMES = {"mdnoconf_cross_rmsd_workspace_bytes", "mdnoconf_cross_rmsd"}
FAKE = 0x10000          # a made-up address: nothing may dereference it
BIG = 1 << 62


def test_conformations_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    assert set(_lib.CONFORMATIONS_SIGNATURES) == NAMES
    assert lib.mdno_abi_version() == 15 == _lib.ABI_VERSION and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "conformations.hip").exists() and (CSRC / "superpose.h").exists()      # inside the library's content hash
    text = HEADER.read_text()
    assert int(re.search(r"#define MDNO_CONF_FRAME_TILE (\d+)", text).group(1)) == ops.CONF_FRAME_TILE
    assert int(re.search(r"#define MDNO_CONF_ATOM_CHUNK (\d+)", text).group(1)) == ops.CONF_ATOM_CHUNK
    assert "mdnoconf_" in text and "prefix" in text.lower()                               # the header says why the names differ


def test_the_eigen_solve_has_one_definition():
    """rmsd2_from_moments lives in csrc/superpose.h alone; forecast.hip and conformations.hip include it."""
    holders = [f.name for f in sorted(CSRC.iterdir()) if f.suffix in (".hip", ".h")
               and re.search(r"double\s+rmsd2_from_moments\s*\(", f.read_text())]
    assert holders == ["superpose.h"]
    for name in ("forecast.hip", "conformations.hip"):
        text = (CSRC / name).read_text()
        assert '#include "superpose.h"' in text and "rmsd2_from_moments(" in text


def call(lib, a=FAKE, S=3, M=2, b=FAKE, Fb=5, N=4, matrix=FAKE, nearest=FAKE, nearest_index=FAKE, cover=FAKE, cover_step=FAKE,
         ws=FAKE, ws_bytes=BIG):
    return lib.mdnoconf_cross_rmsd(a, S, M, b, Fb, N, matrix, nearest, nearest_index, cover, cover_step, ws, ws_bytes, None)


def test_entry_point_refuses_before_device_work(lib):
    """No pointer below is a device pointer: a call that got as far as a launch would fault, not return a code."""
    from molecular_dynamics_neural_operator_amd import _lib
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED
    err = lib.mdno_last_error
    for kw in ({"S": -1}, {"M": -1}, {"N": -1}, {"Fb": -1}):
        assert call(lib, **kw) == E, kw
    # half a pair of outputs
    for kw in ({"nearest": None}, {"nearest_index": None}, {"cover": None}, {"cover_step": None}):
        assert call(lib, **kw) == E and b"go together" in err(), kw
    # all outputs null
    assert call(lib, matrix=None, nearest=None, nearest_index=None, cover=None, cover_step=None) == E and b"no output" in err()
    # a null input with work to do
    for kw in ({"a": None}, {"b": None}):
        assert call(lib, **kw) == E and b"null pointer" in err(), kw
    # the workspace: null or short, for the outputs asked for
    for want_cover in (0, 1):
        need = lib.mdnoconf_cross_rmsd_workspace_bytes(3, 2, 4, 5, want_cover)
        assert need >= (6 + 5) * 5 * 8
        kw = {} if want_cover else {"cover": None, "cover_step": None}
        assert call(lib, ws_bytes=need - 1, **kw) == E and b"workspace" in err()
        assert call(lib, ws=None, **kw) == E and b"workspace" in err()
        assert call(lib, ws_bytes=0, **kw) == E
    assert lib.mdnoconf_cross_rmsd_workspace_bytes(3, 2, 4, 5, 1) > lib.mdnoconf_cross_rmsd_workspace_bytes(3, 2, 4, 5, 0)
    # M x row tiles x column tiles beyond the launch grid
    assert call(lib, S=1 << 20, M=1 << 10, Fb=1 << 30) == U and b"grid" in err()
    assert call(lib, S=32, M=1, Fb=32 * ((1 << 31) - 1)) == U and b"grid" in err()
    assert call(lib, S=(1 << 31) - 1, M=(1 << 31) - 1, Fb=1 << 62) == U
    # (the argument checks come first)
    assert call(lib, S=1 << 20, M=1 << 10, Fb=1 << 30, nearest=None) == E
    # nothing to compare and no output with a counterpart: returns 0 and looks at nothing, whatever the pointers
    assert call(lib, S=0, Fb=0, a=None, b=None, ws=None, ws_bytes=0) == 0
    assert call(lib, S=0, Fb=0, M=0, a=None, b=None, ws=None, ws_bytes=0) == 0
    assert call(lib, S=0, Fb=7, M=0, a=None, b=None, ws=None, ws_bytes=0) == 0                      # [0, 0] and [0, 7]: empty
    assert call(lib, S=0, Fb=7, a=None, b=None, nearest=None, nearest_index=None, cover=None, cover_step=None, ws=None,
                ws_bytes=0) == 0                                                                    # the matrix is empty
    assert call(lib, S=0, Fb=0, N=-1) == E and call(lib, S=0, Fb=0, cover=None) == E


def test_workspace_bytes_are_monotone(lib):
    from molecular_dynamics_neural_operator_amd import ops
    f = lib.mdnoconf_cross_rmsd_workspace_bytes
    T = ops.CONF_FRAME_TILE
    base = dict(S=100, M=8, N=300, Fb=70)
    for want_cover in (0, 1):
        b0 = f(*base.values(), want_cover)
        assert b0 >= (100 * 8 + 70) * 5 * 8 + 100 * 8 * -(-70 // T) * 12
        for key in base:
            prev = 0
            for scale in (1, 2, 3, 7, 40, 128):
                args = dict(base)
                args[key] = base[key] * scale
                cur = f(*args.values(), want_cover)
                assert cur >= prev and cur >= b0, (key, scale)
                prev = cur
        assert f(*base.values(), 1) >= b0
    assert f(*base.values(), 1) - f(*base.values(), 0) >= 8 * -(-100 // T) * 70 * 12
    assert f(-1, 8, 300, 70, 1) == 0 and f(100, 8, 300, -1, 1) == 0 and f(100, 8, 0, 70, 1) > 0
    assert f(0, 8, 300, 70, 1) <= f(1, 8, 300, 70, 1) and f(100, 8, 300, 0, 1) <= f(100, 8, 300, 1, 1)
    assert f((1 << 31) - 1, (1 << 31) - 1, 5, 1 << 62, 1) == (1 << 64) - 1                 # does not fit: saturates
    # the benchmark's shape: 64 members x 1,000 steps against 1,000 frames stays far below the matrix itself (512 MB)
    assert f(1000, 64, 504, 1000, 1) < 64 * 1024 * 1024


def test_python_arguments_are_checked_without_a_device():
    from molecular_dynamics_neural_operator_amd import forecast, ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    x, y = torch.zeros(6, 4, 5, 3), torch.zeros(7, 5, 3)
    for fn in (lambda: ops.cross_rmsd(x, y), lambda: forecast.cross_rmsd(x, y), lambda: forecast.cross_rmsd(x[:, 0], y, matrix=False)):
        with pytest.raises(MdnoError, match="CPU tensor"):
            fn()
    with pytest.raises(MdnoError, match="torch tensor"):
        ops.cross_rmsd(x.numpy(), y)


def test_cross_rmsd_arithmetic_on_closed_form_toys():
    """CrossRmsd on hand-written fields: S = 4 steps, M = 2 members, Fb = 3 reference frames.  Member 1's step 2 is invalid
    (NaN, -1) and reference frame 2 is invalid (its column NaN, never chosen)."""
    from molecular_dynamics_neural_operator_amd.forecast import CrossRmsd
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    nan = float("nan")
    matrix = torch.tensor([[[0.5, 2.0, nan], [3.0, 1.0, nan]],
                           [[1.5, 0.25, nan], [4.0, 5.0, nan]],
                           [[2.5, 2.5, nan], [nan, nan, nan]],
                           [[0.5, 3.0, nan], [0.75, 6.0, nan]]], dtype=torch.float64)
    r = ref.Result(matrix.numpy() ** 2, np.ones((4, 2, 3)))
    c = CrossRmsd(matrix, torch.from_numpy(r.nearest), torch.from_numpy(r.nearest_index), torch.from_numpy(r.cover),
                  torch.from_numpy(r.cover_step))
    assert c.nearest_index.tolist() == [[0, 1], [1, 0], [0, -1], [0, 0]]                   # 2.5 == 2.5: the lowest index
    assert c.cover_step.tolist() == [[0, 1, -1], [3, 0, -1]]                               # 0.5 at steps 0 and 3: the lowest
    assert c.nearest[:, 0].tolist() == [0.5, 0.25, 2.5, 0.5] and c.cover[0, :2].tolist() == [0.5, 0.25]
    assert c.precision(0.5).tolist() == [0.75, 0.0] and c.precision(1.0).tolist() == [0.75, 2.0 / 3.0]
    assert c.precision(10.0).tolist() == [1.0, 1.0]                                        # of the VALID frames: 4 and 3
    assert c.coverage(0.5).tolist() == [1.0, 0.0] and c.coverage(0.75).tolist() == [1.0, 0.5] and c.coverage(1.0).tolist() == [1.0, 1.0]
    assert torch.equal(c.to_reference(1).contiguous().view(torch.int64), matrix[:, :, 1].contiguous().view(torch.int64))
    parts = [CrossRmsd(matrix[:, m:m + 1], c.nearest[:, m:m + 1], c.nearest_index[:, m:m + 1], c.cover[m:m + 1], c.cover_step[m:m + 1])
             for m in range(2)]
    j = CrossRmsd.cat(parts)
    for name in ("matrix", "nearest", "nearest_index", "cover", "cover_step"):
        a, b = getattr(j, name), getattr(c, name)
        assert a.shape == b.shape and torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), name
    none = CrossRmsd(None, c.nearest, c.nearest_index, c.cover, c.cover_step)
    with pytest.raises(MdnoError, match="matrix"):
        none.to_reference(0)
    with pytest.raises(MdnoError, match="matrix"):
        CrossRmsd.cat([none, c])
    assert CrossRmsd.cat([none, none]).matrix is None and none.cpu().matrix is None
    # a member without any valid frame, a run without any valid reference: NaN, not a division by zero
    dead = CrossRmsd(None, torch.full((3, 1), nan, dtype=torch.float64), torch.full((3, 1), -1), torch.full((1, 2), nan, dtype=torch.float64),
                     torch.full((1, 2), -1))
    assert torch.isnan(dead.precision(1.0)).all() and torch.isnan(dead.coverage(1.0)).all()


def test_lowest_index_rule_of_the_restatement():
    v = np.array([[3.0, 1.0, 1.0, np.nan], [np.nan, np.nan, np.nan, np.nan], [np.nan, 2.0, 5.0, 2.0]])
    val, idx = ref.lowest_min(v, 1)
    assert idx.tolist() == [1, -1, 1] and val[0] == 1.0 and np.isnan(val[1]) and val[2] == 2.0
    val, idx = ref.lowest_min(v, 0)
    assert idx.tolist() == [0, 0, 0, 2] and val.tolist() == [3.0, 1.0, 1.0, 2.0]
    val, idx = ref.lowest_min(np.zeros((2, 0)), 1)
    assert idx.tolist() == [-1, -1] and np.isnan(val).all()


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 15, 16, 17, 28, 63, 64, 65, 129, 504])
def test_the_restatement_agrees_with_explicit_kabsch_inside_the_gate(N):
    """The eigenvalue route against the SVD route on the stacked families (noise 1e-6 to 3, rotations, mirror images, planar
    and collinear frames, an offset of 1e3, identical frames and exact rigid copies), and on plain noise 0 to 5."""
    A, B, ka, kb = ref.stacked(3, 2, N, 9, seed=N)
    rng = np.random.default_rng(1000 + N)
    extra = np.stack([A[0, 0].astype(np.float64) @ ref.rotation(rng).T + rng.normal(scale=s, size=(N, 3)) for s in (0.0, 0.5, 5.0)])
    B = np.concatenate([B, extra.astype(np.float32)])
    r = ref.cross_rmsd(A, B)
    worst = 0.0
    for s in range(3):
        for m in range(2):
            for j in range(B.shape[0]):
                want, G = ref.superpose_rmsd2(A[s, m], B[j])
                assert abs(G - r.G[s, m, j]) <= (3 * N + 4) * 2.0 ** -53 * G         # two orders of a 3 N-term sum
                assert abs(r.matrix2[s, m, j] - want) <= ref.GATE * G, (N, s, m, j, ka[s][m])
                worst = max(worst, abs(r.matrix2[s, m, j] - want) / G if G > 0 else 0.0)
    print(f"N={N}: eigenvalue route against Kabsch, largest |d rmsd^2| / (2^-52 G) = {worst / ref.U52:.3f} (allowed 8)")
    assert r.matrix2[0, 0, 0] <= ref.GATE * r.G[0, 0, 0]                                   # identical
    assert r.matrix2[0, 0, 1] <= ref.GATE * r.G[0, 0, 1]                                   # the exact rigid copy
    if N >= 5:
        assert r.matrix2[0, 0, 2] * N > 1e-2 * r.G[0, 0, 2]                                # a mirror image is NOT small
