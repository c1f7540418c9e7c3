"""csrc/philox.h without a GPU: the numpy restatement (tests/philox_ref.py) reproduces the published Philox4x32-10
known-answer vectors; philox.h compiled for the host gives the restatement's words bit for bit; the names of
include/mdno_noise.h's table are pinned (tests/test_cabi_tables.py holds header, table and exports together), and the entry points validate before any device work."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import philox_ref as P
from cabi import CSRC, lib  # noqa: F401  (lib: the fixture)

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, expected
KAT = [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_restatement_reproduces_known_answer_vectors():
    for ctr, key, want in KAT:
        got = " ".join(f"{int(w):08x}" for w in P.philox4x32_10(ctr, key))
        assert got == want, (ctr, key)
    # vectorised over leading dimensions = one at a time
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint64)
    keys = np.array([k[1] for k in KAT], dtype=np.uint64)
    assert [" ".join(f"{int(w):08x}" for w in row) for row in P.philox4x32_10(ctrs, keys)] == [k[2] for k in KAT]


def test_counter_layout_and_uniforms():
    """What a value depends on: every field of (seed, stream, index, element, purpose) changes the words, index 2^40 is
    not index 0, and the word is purpose (| 0x100) alone below 2^32; u in (0, 1]."""
    base = P.noise_words(7, [3], 5, 12, P.ROLLOUT)
    for other in (P.noise_words(8, [3], 5, 12, 0), P.noise_words(7 + 2 ** 32, [3], 5, 12, 0), P.noise_words(7, [4], 5, 12, 0),
                  P.noise_words(7, [3], 6, 12, 0), P.noise_words(7, [3], 5 + 2 ** 40, 12, 0), P.noise_words(7, [3], 5, 12, 1)):
        assert not np.array_equal(base, other)
    blk = P.philox4x32_10([3, 5, 2, 0], [7, 0])
    blk2 = P.philox4x32_10([3, 5, 2, 0x100], [7, 0])
    assert np.array_equal(base[0, 8:12, 0], blk) and np.array_equal(base[0, 8:12, 1], blk2)
    assert np.array_equal(base[0, :8], P.noise_words(7, [3], 5, 8, 0)[0])          # a prefix does not depend on the length
    u = P.uniform32(np.array([0, 255, 256, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and float(u[0]) == float(u[1]) == 2.0 ** -25 and float(u[2]) == 1.5 * 2.0 ** -24
    assert float(u[3]) == 1.0
    z = P.normals(P.noise_words(1, [0, 1], 0, 3000, 0))
    assert np.isfinite(z).all() and np.abs(z).max() < 6.0


def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler (c++, g++, clang++ or $CXX) on PATH")


HOST_MAIN = r"""
#include <cstdio>
#include "philox.h"
int main() {
    char kind;
    unsigned long long a[7];
    while (scanf(" %c %llu %llu %llu %llu %llu %llu", &kind, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 7) {
        uint32_t w[4];
        if (kind == 'R') {          // raw block: c0 c1 c2 c3 k0 k1
            for (int i = 0; i < 4; ++i) w[i] = (uint32_t)a[i];
            mdno::philox4x32_10(w, (uint32_t)a[4], (uint32_t)a[5]);
        } else {                    // noise block: seed stream index block purpose second
            mdno::noise_block(a[0], (uint32_t)a[1], (long long)a[2], (uint32_t)a[3], (int)a[4], (int)a[5], w);
        }
        printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    }
    return 0;
}
"""


def test_philox_header_compiled_for_the_host(tmp_path):
    """philox.h in a stand-alone host program (system compiler, no HIP): 1,000 random raw counters and 200 blocks of
    the library's counter layout (64-bit seeds, indices up to 2^48, both purposes) give the restatement's words."""
    (tmp_path / "main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "philox_host"
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), str(tmp_path / "main.cpp"),
                    "-o", str(exe), "-lm"], check=True)
    rng = np.random.default_rng(20240)
    raw = rng.integers(0, 2 ** 32, size=(1000, 6), dtype=np.uint64)
    raw[0], raw[1] = 0, 0xFFFFFFFF
    nb = np.stack([rng.integers(0, 2 ** 64, size=200, dtype=np.uint64), rng.integers(0, 2 ** 31, size=200, dtype=np.uint64),
                   rng.integers(0, 2 ** 48, size=200, dtype=np.uint64), rng.integers(0, 2 ** 30, size=200, dtype=np.uint64),
                   rng.integers(0, 2, size=200, dtype=np.uint64), rng.integers(0, 2, size=200, dtype=np.uint64)], axis=1)
    nb[:50, 2] = rng.integers(0, 2 ** 32, size=50, dtype=np.uint64)
    text = "".join("R " + " ".join(str(int(v)) for v in r) + "\n" for r in raw) + \
           "".join("B " + " ".join(str(int(v)) for v in r) + "\n" for r in nb)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([[int(w, 16) for w in line.split()] for line in out if line], dtype=np.uint32)
    assert got.shape == (1200, 4)
    assert np.array_equal(got[:1000], P.philox4x32_10(raw[:, :4], raw[:, 4:]))
    assert " ".join(f"{int(w):08x}" for w in got[0]) == KAT[0][2] and " ".join(f"{int(w):08x}" for w in got[1]) == KAT[1][2]
    for row, (seed, sid, index, block, purpose, second) in zip(got[1000:], nb.tolist()):
        words = P.noise_words(seed, [sid], index, 4 * block + 4, purpose)[0, 4 * block:, second] if block < 64 else None
        word3 = purpose | (second << 8) | ((index >> 32) << 16)
        want = P.philox4x32_10([sid, index & 0xFFFFFFFF, block, word3], [seed & 0xFFFFFFFF, seed >> 32])
        assert np.array_equal(row, want)
        if words is not None:
            assert np.array_equal(row, words)


# ------------------------------------------------------------------------------------------------ header, table, exports
def test_noise_header_table_and_exports_agree(lib):
    """What is particular to this header; that header, table and exports agree is tests/test_cabi_tables.py's."""
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(_lib.NOISE_SIGNATURES) == {"mdno_noise_fill", "mdno_noise_add_window", "mdno_rollout_plan_set_noise"}
    assert lib.mdno_abi_version() == 15 and lib.mdno_train_abi_version() == 1          # additive: both stay
    assert (CSRC / "philox.h").exists() and (CSRC / "noise.hip").exists()              # inside the library's content hash


def test_noise_entry_points_validate_before_device_work(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    E = _lib.EINVAL
    assert lib.mdno_noise_fill(0, None, 1, 0, 5, 15, 0, 1.0, None, None, None) == E and b"null pointer" in lib.mdno_last_error()
    assert lib.mdno_noise_fill(0, None, 1, 0, 5, 14, 0, 1.0, None, None, None) == E          # not a multiple of 3 N
    assert lib.mdno_noise_fill(0, None, 1, 2 ** 48, 5, 15, 0, 1.0, None, None, None) == E and b"2^48" in lib.mdno_last_error()
    assert lib.mdno_noise_fill(0, None, 1, -1, 5, 15, 0, 1.0, None, None, None) == E
    assert lib.mdno_noise_fill(0, None, 1, 0, 5, 15, 256, 1.0, None, None, None) == E
    assert lib.mdno_noise_fill(0, None, 0, 0, 5, 15, 0, 1.0, None, None, None) == 0          # nothing to do
    assert lib.mdno_noise_add_window(0, None, None, 2, 3, 10, 5, 0, 1.0, None, None, None) == E
    assert b"null pointer" in lib.mdno_last_error()
    assert lib.mdno_noise_add_window(0, None, None, 2, 3, 10, 11, 0, 1.0, None, None, None) == E      # rows per sample > R
    assert lib.mdno_noise_add_window(0, None, None, 2, 3, 10, 5, 2 ** 48, 1.0, None, None, None) == E
    assert lib.mdno_noise_add_window(0, None, None, 0, 3, 10, 5, 0, 1.0, None, None, None) == 0
    assert lib.mdno_rollout_plan_set_noise(None, 0.1, 0, None) == E and b"null plan" in lib.mdno_last_error()


def test_python_arguments_are_checked_without_a_device():
    import torch
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import MdnoError
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    from molecular_dynamics_neural_operator_amd.training import add_window_noise
    with pytest.raises(MdnoError, match="sample"):
        add_window_noise(PairData(x_position=torch.zeros(3, 4, 3)), 0.1)
    with pytest.raises(MdnoError):
        ops._noise_seed(-1)
    with pytest.raises(MdnoError):
        ops._noise_ids([0, 2 ** 31], "cpu", "stream_ids")
    assert ops._noise_ids([0, 5, 2 ** 31 - 1], "cpu", "stream_ids").dtype == torch.int32
