"""The factored conv's output, bit for bit what it was before K2 on two fp16 planes began to add a chain's four slices
itself (csrc/moment.hip: project_f16_kernel stores 32 chain partials, finish_kernel<1> adds them; the other GEMM modes
keep the 128 slice partials and finish_kernel<4>).

tests/golden/factored_conv_bits.npz holds the raw uint32 images of the last conv application's output (the forward's
`latent`), recorded by scripts/record_factored_conv_bits.py on the commit BEFORE that change, through the same op
test_factored_conv_matches_materialized_and_reference calls (ops.kernelnn_forward, conv_mode "factored").  Every input
is built here from numpy.random.default_rng with fixed seeds; the recording script imports this file for them.

The shapes are the smallest at which the chain indexing can go wrong: R = 1, 63, 64, 65 (a partial last group of 64
rows, the group boundary, rows past the count clamped), 257 (a last group of one row behind four whole ones), 504 (the
benchmark's rows), 600 (two chunks of 512); k = 128 (a slice of 2 k-tiles, slice 127 of 4: the shortest loop, no whole
round of register sets for the last chain's tail), 384 (not a power of two) and 1024.  From 63 rows on every graph has a
destination without in-edges, a hub of in-degree 320, and one destination whose in-edges carry attributes 16 times the
others' — its row of S, like the hub's, has another scale than its neighbours', so a wrong row-exponent index shows.
`aggr` is "mean" and root / bias are present in every forward the C ABI can express (mdno_kernelnn_fwd and
mdno_train_moment_fwd pass MDNO_AGGR_MEAN and require both pointers): "add" and the null pointers cannot be reached
from a test, K3's code behind the chain sum is what it was, and the nearest expressible case — root and bias all zero —
is here."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GOLDEN_FILE = GOLDEN / "factored_conv_bits.npz"

# (rows, ker_width, gemm_mode, variant)
CASES = [(r, 128, "split_f16", "") for r in (1, 63, 64, 65, 257, 504, 600)] + [
    (65, 384, "split_f16", ""), (65, 1024, "split_f16", ""), (257, 1024, "split_f16", ""),
    (65, 128, "split_f16", "zero_root_bias"),
    (257, 128, "split_bf16", ""), (65, 384, "split_bf16", ""),
    (257, 128, "f32", ""), (65, 384, "f32", ""),
]


def case_id(case):
    r, k, mode, variant = case
    return f"R{r}-k{k}-{mode}" + (f"-{variant}" if variant else "")


def case_inputs(case):
    """-> (state_dict, frames [W, 1, R, 3], amino acids [R], edge_index [2, E], edge_attr [E, 6]) of a case."""
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    r, k, _, variant = case
    rng = np.random.default_rng([r, k, 20261020])
    sd = near_identity_state_dict(64, k, seed=r + k, kernel_gain=3e-2, feature_gain=0.3, kernel_to_coords=1.0)
    sd = {key: v.to(torch.float32) for key, v in sd.items()}
    for key in ("conv1.root", "conv2.root", "conv1.bias", "conv2.bias"):      # every entry live, both signs
        sd[key] = torch.from_numpy((rng.standard_normal(tuple(sd[key].shape)) * 0.2).astype(np.float32))
        if variant == "zero_root_bias":
            sd[key] = torch.zeros_like(sd[key])
    frames = (rng.standard_normal((10, 1, r, 3)) * 4).astype(np.float32)
    aa = rng.integers(0, 20, size=r)
    e = 40 if r == 1 else 2000 + 4 * r
    ei = rng.integers(0, r, size=(2, e))
    ea = (rng.standard_normal((e, 6)) * 3).astype(np.float32)
    if r >= 63:
        ei[1, :320] = 11                       # a hub: in-degree >= 320
        ei[1, ei[1] == 3] = 4                  # destination 3: no in-edge
        ea[ei[1] == 7] *= 16.0                 # destination 7: a row of S on another scale than rows 6 and 8
        assert (ei[1] == 11).sum() > 300 and not (ei[1] == 3).any() and (ei[1] == 7).any()
    return sd, frames, aa, ei, ea


def run_case(case, dev):
    """The forward of a case -> the uint32 image of its latent [R, 64] (the last conv application's output)."""
    from molecular_dynamics_neural_operator_amd import ops
    r, k, mode, _ = case
    sd, frames, aa, ei, ea = case_inputs(case)
    pack = ops.ParamPack(sd, 1, dev, gemm_mode=mode, conv_mode="factored")
    g = ops.coo_to_csr(torch.from_numpy(ei).to(dev), r)
    assert ops._lib.load().mdno_resolve_conv_mode(pack.ref, 1, g.edge_cap) == ops._lib.CONV_MODES["factored"]
    _, lat = ops.kernelnn_forward(pack, torch.from_numpy(frames).to(dev), torch.from_numpy(aa), g,
                                  edge_attr=torch.from_numpy(ea).to(dev), return_latent=True)
    lat = lat.cpu().numpy()
    assert lat.shape == (r, 64) and np.isfinite(lat).all() and np.abs(lat).max() > 0
    return lat.view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN_FILE) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_factored_conv_bits_are_the_recorded_ones(dev, recorded, case):
    want = recorded[case_id(case)]
    got = run_case(case, dev)
    differing = int((got != want).sum())
    print(f"{case_id(case)}: {differing} of {got.size} words differ")
    assert np.array_equal(got, want)
