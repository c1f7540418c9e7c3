"""csrc/rigid_rule.h without a GPU: compiled into a stand-alone host program it gives the numpy restatement
(tests/rigid_ref.py) bit for bit — quaternion, translation, the nine matrix entries, the accepted elements; the restatement
is a proper rotation and uniform over SO(3); the Python arguments are checked before any device work.  That header, table
and exports agree is tests/test_cabi_tables.py's."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rigid_ref as RR
from cabi import CSRC, lib  # noqa: F401  (lib: the fixture)

SEEDS = (2024, 0x9E3779B97F4A7C15)
EPOCHS = (0, 3, 2 ** 40 + 5)
LASTS = (65, 3)
SAMPLES = range(64)
TRANSLATE = 2.5


def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler (c++, g++, clang++ or $CXX) on PATH")


HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "rigid_rule.h"
static unsigned long long bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
int main() {
    unsigned long long seed, sample, epoch;
    int last;
    double T;
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'C') {          // centroid: N, then 3 N coordinates as fp32 bit patterns
            int N;
            if (scanf("%d", &N) != 1) return 1;
            std::vector<float> x(3 * (size_t)N);
            for (auto& v : x) {
                unsigned u;
                if (scanf("%x", &u) != 1) return 1;
                memcpy(&v, &u, 4);
            }
            double c[3];
            mdno::rigid_centroid(x.data(), N, c);
            printf("%016llx %016llx %016llx\n", bits(c[0]), bits(c[1]), bits(c[2]));
            continue;
        }
        if (scanf("%llu %llu %llu %d %lf", &seed, &sample, &epoch, &last, &T) != 5) return 1;
        double q[4], t[3], R[9];
        int att[2];
        mdno::rigid_quaternion(seed, (uint32_t)sample, (long long)epoch, last, q, att);
        mdno::rigid_shift(seed, (uint32_t)sample, (long long)epoch, T, t);
        mdno::rigid_matrix(q, R);
        for (int i = 0; i < 4; ++i) printf("%016llx ", bits(q[i]));
        for (int i = 0; i < 3; ++i) printf("%016llx ", bits(t[i]));
        for (int i = 0; i < 9; ++i) printf("%016llx ", bits(R[i]));
        printf("%08x %08x\n", (unsigned)att[0], (unsigned)att[1]);
    }
    return 0;
}
"""


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_seed_2024_samples_reach_every_branch():
    """What the cases below rest on, stated on the restatement first: at seed 2024, epoch 0, some of samples 0..63 reject
    before their first acceptance, some between the two, none needs an element past 7 — so last_element = 3 reaches the
    fallback on real samples and 65 never does."""
    m = RR.motions(2024, SAMPLES, 0)
    first, second = m["attempts"][:, 0], m["attempts"][:, 1]
    assert (first >= 2).all() and (second > first).all()                    # no fallback at 65
    assert int((first > 2).sum()) == 15 and int((second > first + 1).sum()) == 12 and int(second.max()) <= 7
    short = RR.motions(2024, SAMPLES, 0, last_element=3)
    fell = short["attempts"][:, 1] < 0
    assert fell.any() and not fell.all()
    assert np.array_equal(fell, second > 3)
    assert (short["quaternion"][fell] == [1.0, 0.0, 0.0, 0.0]).all()
    assert np.array_equal(_bits(short["quaternion"][~fell]), _bits(m["quaternion"][~fell]))
    assert (short["attempts"][fell, 0] == np.where(first[fell] <= 3, first[fell], -1)).all()


def test_rigid_rule_compiled_for_the_host(tmp_path):
    """rigid_rule.h in a stand-alone host program (system compiler, no HIP, -ffp-contract=off as the library is built):
    2 seeds x 64 samples x 3 epochs x last_element 65 and 3, every printed word equal to the restatement's; and the
    centroid of nine frames in the header's summation order."""
    (tmp_path / "main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "rigid_host"
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", str(CSRC),
                    str(tmp_path / "main.cpp"), "-o", str(exe), "-lm"], check=True)
    cases = [(seed, epoch, last) for seed in SEEDS for epoch in EPOCHS for last in LASTS]
    text = "".join(f"M {seed} {s} {epoch} {last} {TRANSLATE}\n" for seed, epoch, last in cases for s in SAMPLES)
    sizes = (1, 2, 3, 28, 63, 64, 65, 257, 1025)                      # the centroid's order: its tails and whole rounds
    frames = [(np.random.default_rng(n).standard_normal((n, 3)) * 10.0 + (30.0, -12.0, 5.0)).astype(np.float32) for n in sizes]
    text += "".join(f"C {len(f)} " + " ".join(f"{int(w):x}" for w in f.view(np.uint32).reshape(-1)) + "\n" for f in frames)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [line.split() for line in out if line]
    centroids, rows = rows[-len(sizes):], rows[:-len(sizes)]
    for f, row in zip(frames, centroids):
        assert np.array_equal(np.array([int(w, 16) for w in row], dtype=np.uint64), _bits(RR.centroid(f, len(f))[0])), len(f)
    assert len(rows) == len(cases) * 64 and all(len(r) == 18 for r in rows)
    got = np.array([[int(w, 16) for w in r[:16]] for r in rows], dtype=np.uint64).reshape(len(cases), 64, 16)
    att = np.array([[struct.unpack("i", struct.pack("I", int(w, 16)))[0] for w in r[16:]] for r in rows],
                   dtype=np.int32).reshape(len(cases), 64, 2)
    for i, (seed, epoch, last) in enumerate(cases):
        m = RR.motions(seed, SAMPLES, epoch, translate=TRANSLATE, last_element=last)
        what = (hex(seed), epoch, last)
        assert np.array_equal(got[i, :, 0:4], _bits(m["quaternion"])), what
        assert np.array_equal(got[i, :, 4:7], _bits(m["shift"])), what
        assert np.array_equal(got[i, :, 7:16], _bits(RR.matrices(m["quaternion"]).reshape(64, 9))), what
        assert np.array_equal(att[i], m["attempts"]), what
    assert (att[1, :, 1] < 0).any() and (att[0] >= 0).all()          # the fallback was reached at 3, never at 65


def test_the_restatement_is_a_proper_rotation():
    """R R^T = I and det R = 1 within 8 x 2^-52 over 4096 samples (q is not normalised: g = 2 / |q|^2 does it)."""
    q = RR.motions(2024, range(4096), 1)["quaternion"]
    assert np.abs((q * q).sum(1) - 1.0).max() < 1e-15
    R = RR.matrices(q)
    eye = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    det = np.abs(np.linalg.det(R) - 1.0).max()
    print("max |R R^T - I|", eye, "max |det R - 1|", det)
    assert eye <= 8 * 2.0 ** -52 and det <= 8 * 2.0 ** -52
    # any q != 0 gives a rotation: scaled by 3 and by 1e-3 the matrix is the same within rounding
    for scale in (3.0, 1e-3):
        assert np.abs(RR.matrices(q * scale) - R).max() <= 8 * 2.0 ** -52


def test_the_restatement_is_uniform():
    """Over samples 0..4095 every entry of the mean of R lies within 5 standard deviations of zero: an entry of a Haar
    rotation has mean 0 and variance 1/3, so the bound is 5 / sqrt(3 x 4096) = 0.045."""
    R = RR.matrices(RR.motions(2024, range(4096), 0)["quaternion"])
    mean = R.mean(0)
    print(mean)
    assert np.abs(mean).max() < 5.0 / np.sqrt(3 * 4096)
    t = RR.motions(2024, range(4096), 0, rotate=False, translate=2.0)
    assert (t["quaternion"] == [1.0, 0.0, 0.0, 0.0]).all() and (t["attempts"] == -1).all()
    assert np.abs(t["shift"]).max() <= 2.0 and np.abs(t["shift"].mean(0)).max() < 5.0 * 2.0 / np.sqrt(3 * 4096)
    zero = RR.motions(2024, range(64), 0, translate=0.0)["shift"]
    assert (zero == 0.0).all()


# ------------------------------------------------------------------------------------------------ arguments
def test_augment_header_names_and_purpose(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.AUGMENT_SIGNATURES) == {"mdnoaug_motions", "mdnoaug_apply", "mdnoaug_edge_attr"}
    assert _lib.NOISE_PURPOSES == {"rollout": 0, "train_window": 1, "train_motion": 2}
    assert lib.mdno_abi_version() == 15 and lib.mdno_train_abi_version() == 1          # additive: both stay
    header = (CSRC.parents[1] / "include" / "mdno_augment.h").read_text()
    assert "#define MDNO_NOISE_TRAIN_MOTION 2" in header
    assert "NOISE_TRAIN_MOTION = 2" in (CSRC / "philox.h").read_text()


def test_entry_points_validate_before_device_work(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    ok = (0, None, 1, 0, 1, 0.0, 65, None, 0)
    assert lib.mdnoaug_motions(*ok, None, None, None, None, None) == E and b"null pointer" in lib.mdno_last_error()
    for at, bad in ((2, 65536), (2, -1), (3, 2 ** 48), (3, -1), (4, 2), (5, -1.0), (5, float("inf")), (5, float("nan")),
                    (6, 1), (6, 66)):
        args = list(ok)
        args[at] = bad
        assert lib.mdnoaug_motions(*args, None, None, None, None, None) == E, (at, bad)
    assert lib.mdnoaug_motions(0, None, 0, 0, 1, 0.0, 65, None, 0, None, None, None, None, None) == 0      # nothing to do
    assert lib.mdnoaug_apply(None, None, None, 2, 5, 3, 0, None, None, None) == E and b"null pointer" in lib.mdno_last_error()
    assert lib.mdnoaug_apply(None, None, None, 65536, 5, 3, 0, None, None, None) == E
    assert lib.mdnoaug_apply(None, None, None, 2, 2 ** 20, 2 ** 11, 0, None, None, None) == E and b"2^31" in lib.mdno_last_error()
    assert lib.mdnoaug_apply(None, None, None, 2, -1, 3, 0, None, None, None) == E
    assert lib.mdnoaug_apply(None, None, None, 2, 5, 0, 0, None, None, None) == 0
    assert lib.mdnoaug_edge_attr(None, None, 4, 10, None, None) == E and b"null pointer" in lib.mdno_last_error()
    assert lib.mdnoaug_edge_attr(None, None, -1, 10, None, None) == E
    assert lib.mdnoaug_edge_attr(None, None, 0, 10, None, None) == 0


def test_python_arguments_are_checked_without_a_device():
    import torch
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.training import RigidAugment, RigidMotions, augment_batch, draw_motions
    a = RigidAugment()
    assert (a.seed, a.rotate, a.translate, a.pivot) == (0, True, 0.0, "centroid")
    for kw in (dict(translate=-1.0), dict(translate=float("inf")), dict(translate=float("nan")), dict(pivot="center"),
               dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(MdnoError):
            RigidAugment(**kw)
    host = PairData(x_position=torch.zeros(3, 4, 3))
    with pytest.raises(MdnoError, match="DeviceTrajectory.batch"):
        draw_motions(host, a, 0)
    with pytest.raises(MdnoError, match="DeviceTrajectory.batch"):
        augment_batch(host, a, 0)
    periodic = PairData(x_position=torch.zeros(3, 4, 3))
    periodic.sample_ids, periodic.rows_per_sample, periodic.box = np.array([0]), 4, (20.0, 20.0, 20.0)
    with pytest.raises(MdnoError, match="periodic"):
        draw_motions(periodic, a, 0)
    with pytest.raises(MdnoError, match="RigidAugment"):
        draw_motions(host, "rotate", 0)
    with pytest.raises(MdnoError, match="last_element"):
        ops.rigid_motions(0, [0], 0, last_element=66, device="cpu")
    with pytest.raises(MdnoError, match="translate"):
        ops.rigid_motions(0, [0], 0, translate=-0.5, device="cpu")
    with pytest.raises(MdnoError):
        ops.rigid_motions(0, [0, 1], 0, first_frame=torch.zeros(7, 3), n_atoms=4, device="cpu")       # 7 rows, B * N = 8
    with pytest.raises(MdnoError, match=r"\[\.\.\., B \* N, 3\]"):
        ops.rigid_apply(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64),
                        torch.zeros(2, 3, dtype=torch.float64), 4, torch.zeros(7, 3))
    with pytest.raises(MdnoError, match="edge_index"):
        ops.edge_attr_gather(torch.zeros(4, 3), torch.zeros(3, 5, dtype=torch.long))
    with pytest.raises(MdnoError, match="int64"):
        ops.edge_attr_gather(torch.zeros(4, 3), torch.zeros(2, 5, dtype=torch.int32))
    ident = RigidMotions.identity(3, 4, "cpu")
    assert ident.quaternion.tolist() == [[1.0, 0.0, 0.0, 0.0]] * 3 and ident.n_atoms == 4 and (ident.attempts == -1).all()
    assert torch.equal(ident.matrices(), torch.eye(3, dtype=torch.float64).expand(3, 3, 3))
    R = RigidMotions(torch.from_numpy(RR.motions(2024, range(8), 0)["quaternion"]), torch.zeros(8, 3, dtype=torch.float64),
                     torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 2, dtype=torch.int32), 4).matrices()
    assert np.array_equal(_bits(R.numpy()), _bits(RR.matrices(RR.motions(2024, range(8), 0)["quaternion"])))


def test_data_parallel_shard_passes_augment_as_it_passes_noise():
    import types
    from molecular_dynamics_neural_operator_amd.data_parallel import DataParallelTrainer

    class Source:
        def batch(self, idx, **kw):
            self.idx, self.kw = idx, kw
            return types.SimpleNamespace(y="y")

    src, aug = Source(), object()
    B, own, data, y = DataParallelTrainer._shard(types.SimpleNamespace(rank=1, world=2), [3, 4, 5, 6], src,
                                                 dict(noise_std=0.1, noise_seed=2, epoch=5, augment=aug))
    assert (B, own, y) == (4, 2, "y") and src.idx.tolist() == [5, 6]
    assert src.kw == dict(noise_std=0.1, noise_seed=2, epoch=5, augment=aug)
