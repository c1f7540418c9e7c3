"""The ping-pong bf16 GEMMs (csrc/gemm_bf16.hip: gemm_pp_kernel in its A.W^T, persistent A.W^T and A^T.B forms, and the
128-wide kernels the other shapes fall to) held to EXACT products at every tile, stage-count and slice boundary.

The oracle models nothing about the matrix pipe's summation order.  Operands and bias are integers in [-8, 8] (exact in
bf16), so every product is an integer of magnitude <= 64 and every partial sum, in any order, has magnitude <= 64 K + 8
< 2^24 (asserted per case): no fp32 addition rounds, whatever order the MFMA, the K slices or the slab reduction add in.
The fp32 result therefore EQUALS the fp64 product of the CPU; the bf16 result equals torch's round-to-nearest-even of
relu(exact + bias) bit for bit (above 256 most sums are not representable, and odd multiples are exact ties); the masked
result equals the exact product where the stored activation Y is positive and +0 elsewhere, rounded the same way, with Y
drawn from {-1, -0.0, +0.0, 1, the smallest positive subnormal}.

One non-integer run per family (section 4) holds every ELEMENT to 2 (n + 2) 2^-24 (sum |a||w| + |b|), n = contraction
length + slice count: (n + 2) 2^-24 is the any-order worst case of an fp32 sum, the factor 2 covers an adder that
truncates (the matrix pipe's internal rounding is not documented as round-to-nearest).  Section 5 repeats a subset
inside guard bands under both fill bytes."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
BF16 = torch.bfloat16
LIM = 8                               # operands and bias are integers in [-LIM, LIM]

NT_K = [32, 64, 96, 128, 160, 192, 224, 1024]       # stage counts T = K / 32 = 1 (128-wide kernel), 2 .. 7 and 32
NT_N = [128, 256, 384, 512, 768]                    # 128 and 384: the 128-wide kernels and the unfused mask
NT_ROWS = [1, 127, 128, 129, 255, 256, 257, 511, 513]
PERSIST_CASES = ["a", "b", "c", "d", "e"]
TN_WIDTHS = [(256, 256), (256, 512), (512, 256), (512, 512), (128, 384)]      # the last one: the 128-wide kernel
TN_ROWS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257, 385, 4097, 4100, 4129]
# -1, -0.0, +0.0, 1, the smallest positive subnormal (bits 0x0001) as bf16 bit patterns
Y_BITS = torch.tensor([0xBF80 - 0x10000, 0x8000 - 0x10000, 0x0000, 0x3F80, 0x0001], dtype=torch.int16)

_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    _CACHE.clear()


# ================================================================================================ inputs and oracle
def ints(g, *shape):
    return torch.randint(-LIM, LIM + 1, shape, generator=g).float()


def draw_y(g, rows, n):
    return Y_BITS[torch.randint(0, len(Y_BITS), (rows, n), generator=g)].view(BF16)


def keep_mask(y):
    """y > 0 on the CPU; the same thing read off the bits (sign clear and not zero: the subnormal counts)."""
    m = y.float() > 0
    assert torch.equal(m, y.view(torch.int16) > 0)
    return m


def nt_inputs(seed, rows, N, K):
    """A bf16 [rows,K], the fp32 master W [N,K], bias fp32 [N] (integers) and the stored activation Y bf16 [rows,N]."""
    g = torch.Generator().manual_seed(seed)
    return ints(g, rows, K).to(BF16), ints(g, N, K), ints(g, N), draw_y(g, rows, N)


def nt_expected(a, w, b, y):
    """The four results as the CPU computes them: fp64 product (exact), + bias, relu and one rounding, mask and one
    rounding.  The premise of exactness is checked, not assumed."""
    K = a.shape[1]
    assert 64 * K + 8 < 2 ** 24
    exact = a.double() @ w.double().T
    assert float(exact.abs().max()) <= 64 * K and torch.equal(exact, exact.round())
    biased = exact + b.double()
    zero = torch.zeros((), dtype=torch.float64)
    return {"plain": exact.float(), "biased": biased.float(), "relu_bf16": biased.relu().float().to(BF16),
            "masked": torch.where(keep_mask(y), exact, zero).float().to(BF16)}


def bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32}[t.dtype])


def differ(got, want, bitwise):
    """"" where got equals want (bit for bit, or by value: +0 == -0, NaN differs from everything); otherwise how many
    elements differ and the first of them."""
    want = want.to(got.device)
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    bad = (bits(got) != bits(want)) if bitwise else (got != want)
    n = int(bad.sum())
    if n == 0:
        return ""
    i = tuple(bad.nonzero()[0].tolist())
    return f"{n} of {bad.numel()} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


def persist_enabled():
    return not os.environ.get("MDNO_GEMM_PP_PERSIST", "1").startswith("0")


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8


def persist_shape(name, C):
    """(rows, N, K) of the persistent cases: a — C + 4 tiles, T = 2, one live row in the last row tile; b — T = 3;
    c — 2 C + 1 tiles (one workgroup walks three); d — T = 32; e — T = 4 and a walk that CHANGES ITS BIAS COLUMNS.
    A workgroup walks tiles C / 8 apart inside its XCD's range and a tile's columns are tile % (N / 256), so with
    C = 256 and N / 256 = 1, 2 or 4 (cases a - d) every tile of a walk has the same bias: only an N / 256 that does not
    divide C / 8 makes the next tile's bias prefetch observable (a kernel that kept the previous tile's bias passes
    a - d on 256 compute units)."""
    if name == "e":
        N = next(n for n in (768, 1280, 1792) if (C // 8) % (n // 256))
        return 256 * (C // 2) + 77, N, 128
    return {"a": (256 * (C // 4) + 1, 1024, 64), "b": (256 * (C // 2) + 129, 512, 96),
            "c": (256 * (2 * C) + 255, 256, 160), "d": (256 * (C // 4) + 116, 1024, 1024)}[name]


def persist_inputs(name, C):
    key = ("persist", name, C)
    if key not in _CACHE:
        rows, N, K = persist_shape(name, C)
        _CACHE[key] = nt_inputs(7000 + ord(name), rows, N, K)
    return _CACHE[key]


def persist_expected(name, C):
    key = ("persist_expected", name, C)
    if key not in _CACHE:
        _CACHE[key] = nt_expected(*persist_inputs(name, C))
    return _CACHE[key]


def persist_outputs(dev, name, C):
    """(bf16-output relu result, masked result) of a persistent case on the device."""
    from molecular_dynamics_neural_operator_amd import ops
    a, w, b, y = (t.to(dev) for t in persist_inputs(name, C))
    return ops.linear_bf16(a, w, b, relu=True, out_bf16=True), ops.linear_bf16_relu_bwd(a, w, y)


def trunc_div(a, b):
    return abs(a) // b if a >= 0 else -(abs(a) // b)        # C's division


def tn_stage_counts(rows, n1, n2):
    """tn_slices, slice_rows and the kernel's T = (k1 - k0 + 31) / 32 per slice restated (gemm_tn_pp; C division
    truncates toward zero, so a slice that starts 1 .. 31 rows past the end has T == 0 and later ones T < 0)."""
    tiles = (n1 // 256) * (n2 // 256)
    sl = max(1, min(32, 256 // tiles))
    sl = min(sl, (rows + 127) // 128)
    while -(-rows // sl) * max(n1, n2) * 2 >= 2 ** 31:
        sl += 1
    slice_rows = -(-(-(-rows // sl)) // 32) * 32
    return [trunc_div(min(z * slice_rows + slice_rows, rows) - z * slice_rows + 31, 32) for z in range(sl)]


def tn_inputs():
    if "tn" not in _CACHE:
        g = torch.Generator().manual_seed(4129)
        _CACHE["tn"] = (ints(g, max(TN_ROWS), 512), ints(g, max(TN_ROWS), 512))
    return _CACHE["tn"]


def tn_exact(A, B, rows, n1, n2):
    assert 64 * rows + 8 < 2 ** 24
    want = A[:rows, :n1].double().T @ B[:rows, :n2].double()
    assert float(want.abs().max()) <= 64 * rows
    return want.float()


# ================================================================================================ 1. NT, one tile per workgroup
@pytest.mark.parametrize("K", NT_K)
def test_nt_products_equal_the_integer_product(dev, K):
    """Every N and row count of the table at this K: fp32 output with and without bias equals the fp64 product, the
    relu / bf16 output and the masked output equal its single rounding bit for bit.  Rows 1 .. 513 put 1, 127, 128, 129
    and 255 live rows into the last tile, and the grids have 1, 2, 3, 4, 6 and 9 tiles (fewer than XCDs, and counts
    that are no multiple of 8)."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    lib = _lib.load()
    a, w, b, y = nt_inputs(1000 + K, max(NT_ROWS), max(NT_N), K)
    want = {k: v.to(dev) for k, v in nt_expected(a, w, b, y).items()}
    ad, wd, bd, yd = (t.to(dev) for t in (a, w, b, y))
    for N in NT_N:
        for rows in NT_ROWS:
            assert bool(lib.mdno_linear_bf16_masked_supported(rows, N, K)) == (N % 256 == 0 and K >= 64)   # which kernel
            A, W, B, Y = ad[:rows], wd[:N], bd[:N], yd[:rows, :N].contiguous()
            cut = lambda k: want[k][:rows, :N]
            what = f"rows={rows} N={N} K={K}"
            d = differ(ops.linear_bf16(A, W, B, relu=False, out_bf16=False), cut("biased"), bitwise=False)
            assert not d, f"{what} fp32 + bias: {d}"
            d = differ(ops.linear_bf16(A, W, None, relu=False, out_bf16=False), cut("plain"), bitwise=False)
            assert not d, f"{what} fp32: {d}"
            d = differ(ops.linear_bf16(A, W, B, relu=True, out_bf16=True), cut("relu_bf16"), bitwise=True)
            assert not d, f"{what} relu bf16: {d}"
            d = differ(ops.linear_bf16_relu_bwd(A, W, Y), cut("masked"), bitwise=True)
            assert not d, f"{what} masked: {d}"


# ================================================================================================ 2. NT, persistent form
def persist_checked(dev, name):
    C = cus_of(dev)
    if C < 8:
        pytest.skip("fewer than 8 compute units: no persistent form")
    assert persist_enabled(), "MDNO_GEMM_PP_PERSIST=0 in this process: the persistent form would not run"
    rows, N, K = persist_shape(name, C)
    tiles = -(-rows // 256) * (N // 256)
    assert tiles > C, (name, tiles, C)
    if name == "e":
        assert (C // 8) % (N // 256) != 0, (C, N)      # the second tile of a walk has other bias columns
    return C


@pytest.mark.parametrize("name", PERSIST_CASES)
def test_persistent_nt_equals_the_single_tile_form_and_the_integer_product(dev, name):
    """More tiles than compute units: the bf16-output and masked products take the persistent walk, the fp32-output
    product of the same call does not.  The persistent bits equal torch's rounding of the fp32 output (relu, or the mask
    on the bias-free product), and the fp32 output equals the fp64 product — so all three equal the CPU's."""
    from molecular_dynamics_neural_operator_amd import ops
    C = persist_checked(dev, name)
    a, w, b, y = persist_inputs(name, C)
    want = persist_expected(name, C)
    keep = keep_mask(y).to(dev)
    ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
    biased = ops.linear_bf16(ad, wd, bd, relu=False, out_bf16=False)
    plain = ops.linear_bf16(ad, wd, None, relu=False, out_bf16=False)
    out_bf16, out_masked = persist_outputs(dev, name, C)
    d = differ(out_bf16, biased.relu().to(BF16), bitwise=True)
    assert not d, f"case {name}: persistent relu bf16 against the fp32 output rounded: {d}"
    d = differ(out_masked, torch.where(keep, plain, torch.zeros((), device=dev)).to(BF16), bitwise=True)
    assert not d, f"case {name}: persistent masked against the fp32 output masked and rounded: {d}"
    d = differ(biased, want["biased"], bitwise=False)
    assert not d, f"case {name}: fp32 + bias against fp64: {d}"
    d = differ(plain, want["plain"], bitwise=False)
    assert not d, f"case {name}: fp32 against fp64: {d}"
    # (implied by the four above; kept as direct statements of what the persistent kernel must produce)
    assert not differ(out_bf16, want["relu_bf16"], bitwise=True) and not differ(out_masked, want["masked"], bitwise=True)


def _child(out_dir):
    """Run as a script by the test below, in a fresh process with MDNO_GEMM_PP_PERSIST=0."""
    sys.path.insert(0, str(REPO))
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    assert not persist_enabled()
    dev = torch.device("cuda:0")
    C = cus_of(dev)
    for name in PERSIST_CASES:
        o, m = persist_outputs(dev, name, C)
        torch.save({"bf16": bits(o).cpu(), "masked": bits(m).cpu()}, Path(out_dir) / f"{name}.pt")
    torch.cuda.synchronize()
    print("ok one workgroup per tile")


def test_persistent_switch_off_gives_the_same_bits(dev, tmp_path):
    """MDNO_GEMM_PP_PERSIST is read once per process: a fresh child with the switch at 0 computes cases a - e from the
    same seeds with one workgroup per tile, and the persistent results of this process must have the same bits."""
    C = cus_of(dev)
    for name in PERSIST_CASES:
        persist_checked(dev, name)
    env = dict(os.environ, MDNO_GEMM_PP_PERSIST="0")
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok one workgroup per tile" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    for name in PERSIST_CASES:
        saved = torch.load(tmp_path / f"{name}.pt")
        o, m = persist_outputs(dev, name, C)
        d = differ(bits(o), saved["bf16"], bitwise=False)
        assert not d, f"case {name}: relu bf16, persistent against one workgroup per tile: {d}"
        d = differ(bits(m), saved["masked"], bitwise=False)
        assert not d, f"case {name}: masked, persistent against one workgroup per tile: {d}"


# ================================================================================================ 3. A^T . B
def test_tn_slicing_rule_gives_the_empty_slices_the_cases_rely_on():
    """The restated slicing rule at the 256-wide shapes: rows <= 128 are one slice of T = 1 .. 4; 4100 and 4129 end in
    a slice with T == 0 followed by negative ones; 4097 has negative ones only."""
    for n1, n2 in TN_WIDTHS[:4]:
        for rows in TN_ROWS:
            ts = tn_stage_counts(rows, n1, n2)
            if rows <= 128:
                assert ts == [(rows + 31) // 32]
            else:
                assert len(ts) > 1 and sum(t for t in ts if t > 0) >= (rows + 31) // 32
        for rows in (4100, 4129):
            ts = tn_stage_counts(rows, n1, n2)
            assert 0 in ts and min(ts) < 0, (rows, ts)
        ts = tn_stage_counts(4097, n1, n2)
        assert 0 not in ts and min(ts) < 0, ts
    assert tn_stage_counts(4100, 256, 256)[-6:] == [0, -5, -10, -15, -20, -25]
    assert tn_stage_counts(4097, 256, 256)[-6:] == [-1, -6, -11, -16, -21, -26]
    assert {len(tn_stage_counts(r, 256, 256)) for r in (129, 257, 385, 4100)} == {2, 3, 4, 32}


@pytest.mark.parametrize("n1,n2", TN_WIDTHS)
def test_atb_bf16_equals_the_integer_product(dev, n1, n2):
    """Every row count of the table: one slice of T = 1 .. 4 stages, two and more slices, trailing slices with T == 0
    and T < 0 (each must write its zero slab).  Equal to the fp64 product, and the same bits on a second call."""
    from molecular_dynamics_neural_operator_amd import ops
    A, B = tn_inputs()
    Ad, Bd = A.to(BF16).to(dev), B.to(BF16).to(dev)
    for rows in TN_ROWS:
        a, b = Ad[:rows, :n1].contiguous(), Bd[:rows, :n2].contiguous()
        got = ops.gemm_atb_bf16(a, b)
        d = differ(got, tn_exact(A, B, rows, n1, n2), bitwise=False)
        assert not d, f"rows={rows} ({n1}, {n2}) stage counts {tn_stage_counts(rows, n1, n2) if n1 % 256 == 0 else 'n/a'}: {d}"
        assert not differ(ops.gemm_atb_bf16(a, b), got, bitwise=True), f"rows={rows} ({n1}, {n2}): second call differs"


@pytest.mark.parametrize("n1,n2", [(256, 256), (256, 512)])
def test_atb_split_f16_equals_the_integer_product(dev, n1, n2):
    """The same integers as fp32 through the two-plane fp16 form.  Equality holds by the same argument: a column's scale
    is a power of two that puts its largest entry (<= 8) into [2^13, 2^14), so every scaled entry is an integer of at most
    four significant bits times that power — exact in fp16, the lo plane is zero; the hi . hi slabs hold sa sb times
    integers below 2^24 (at most 2^28 . 4129 < 2^41: no overflow), the cross terms are sums of zeros, adding 2^-11 . 0
    changes nothing, and undoing the two scales multiplies by powers of two.  Nothing rounds."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    lib = _lib.load()
    A, B = tn_inputs()
    Ad, Bd = A.to(dev), B.to(dev)
    for rows in TN_ROWS:
        assert lib.mdno_gemm_atb_split_f16_supported(rows, n1, n2)      # (otherwise gemm_atb takes the fp32 kernel)
        a, b = Ad[:rows, :n1].contiguous(), Bd[:rows, :n2].contiguous()
        got = ops.gemm_atb(a, b, gemm_mode="split_f16")
        d = differ(got, tn_exact(A, B, rows, n1, n2), bitwise=False)
        assert not d, f"rows={rows} ({n1}, {n2}): {d}"
        assert not differ(ops.gemm_atb(a, b, gemm_mode="split_f16"), got, bitwise=True), f"rows={rows}: second call differs"


# ================================================================================================ 4. non-integer operands
def normals(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF16)


def gate_ratio(got, want, gate):
    """max over elements of |got - want| / gate (fp64; 0 where the difference is 0)."""
    err = (got.double().cpu() - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / gate)
    return float(q.max())


def nt_gate(a, w, b, slices=1):
    n = a.shape[1] + slices
    return 2.0 * (n + 2) * 2.0 ** -24 * (a.double().abs() @ w.double().abs().T + b.double().abs())


@pytest.mark.parametrize("K", [96, 1024])
def test_nt_normals_within_the_any_order_gate_per_element(dev, K):
    """rows 257, N 512, T = 3 and 32, bf16-rounded normals: every element of the fp32 output within
    2 (K + 3) 2^-24 (sum |a||w| + |b|) of fp64 on the same rounded operands.  Largest error / gate measured on an
    MI355X: 0.0098 (K = 96), 0.00070 (K = 1024); persistent shape b 0.0104; A^T.B 0.0041 (129 rows), 4.5e-5 (4100)."""
    from molecular_dynamics_neural_operator_amd import ops
    a, w, b = normals(K, 257, K), normals(K + 1, 512, K).float(), normals(K + 2, 512).float()
    want = a.double() @ w.double().T + b.double()
    got = ops.linear_bf16(a.to(dev), w.to(dev), b.to(dev), relu=False, out_bf16=False)
    r = gate_ratio(got, want, nt_gate(a, w, b))
    print(f"NT rows=257 N=512 K={K}: largest error / gate {r:.3g}")
    assert r <= 1.0, r


def test_persistent_nt_normals_within_the_gate_and_equal_to_the_single_tile_form(dev):
    """Shape b (T = 3, persistent) on bf16-rounded normals.  The persistent form has bf16 output only, so the gate is
    applied through the rounding: with v the kernel's fp32 value, |v - want| <= gate and rounding is monotone, hence
    bf16(relu(want - gate)) <= out <= bf16(relu(want + gate)) for every element.  The fp32 output of the same shape (one
    workgroup per tile) is held to the gate itself, and the persistent bits must equal its rounding — the kernel's
    "same MFMAs in the same order per output element"."""
    from molecular_dynamics_neural_operator_amd import ops
    C = persist_checked(dev, "b")
    rows, N, K = persist_shape("b", C)
    a, w, b = normals(11, rows, K), normals(12, N, K).float(), normals(13, N).float()
    want = a.double() @ w.double().T + b.double()
    gate = nt_gate(a, w, b)
    ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
    f32 = ops.linear_bf16(ad, wd, bd, relu=False, out_bf16=False)
    r = gate_ratio(f32, want, gate)
    print(f"NT persistent shape b rows={rows} N={N} K={K}: largest error / gate of the fp32 output {r:.3g}")
    assert r <= 1.0, r
    out = ops.linear_bf16(ad, wd, bd, relu=True, out_bf16=True)
    d = differ(out, f32.relu().to(BF16), bitwise=True)
    assert not d, f"persistent relu bf16 against the fp32 output rounded: {d}"
    lo, hi = (want - gate).relu().float().to(BF16).float(), (want + gate).relu().float().to(BF16).float()
    o = out.float().cpu()
    assert bool(((lo <= o) & (o <= hi)).all()), int(((o < lo) | (o > hi)).sum())


@pytest.mark.parametrize("rows", [129, 4100])
def test_atb_bf16_normals_within_the_any_order_gate_per_element(dev, rows):
    """(256, 512), two slices and 32 slices with empty ones, bf16-rounded normals: every element within
    2 (rows + slices + 2) 2^-24 sum |a||b| of fp64 on the same rounded operands."""
    from molecular_dynamics_neural_operator_amd import ops
    n1, n2 = 256, 512
    a, b = normals(rows, rows, n1), normals(rows + 1, rows, n2)
    want = a.double().T @ b.double()
    n = rows + len(tn_stage_counts(rows, n1, n2))
    gate = 2.0 * (n + 2) * 2.0 ** -24 * (a.double().abs().T @ b.double().abs())
    r = gate_ratio(ops.gemm_atb_bf16(a.to(dev), b.to(dev)), want, gate)
    print(f"TN rows={rows} ({n1}, {n2}): largest error / gate {r:.3g}")
    assert r <= 1.0, r


# ================================================================================================ 5. guard bands
GUARD_NT = [(1, 512, 96), (257, 512, 96)]
GUARD_TN = [(rows, n1, n2) for n1, n2 in ((256, 256), (256, 512)) for rows in (1, 33, 129, 4100)]


def _guard_nt_cases(dev):
    cases = [nt_inputs(5000 + rows, rows, N, K) for rows, N, K in GUARD_NT]
    C = cus_of(dev)
    if C >= 8:
        persist_checked(dev, "a")
        cases.append(persist_inputs("a", C))
    return cases


def _guarded_run(dev, fill):
    from guarded import Guard
    from molecular_dynamics_neural_operator_amd import ops
    A, B = tn_inputs()
    res = []
    with Guard(fill, record_calls=False) as G:
        P = lambda t: G.place(t.to(dev))
        for a, w, b, y in _guard_nt_cases(dev):
            a, w, b, y = P(a), P(w), P(b), P(y)
            res.append(ops.linear_bf16(a, w, b, relu=False, out_bf16=False).cpu())
            res.append(ops.linear_bf16(a, w, b, relu=True, out_bf16=True).cpu())
            res.append(ops.linear_bf16_relu_bwd(a, w, y).cpu())
        G.verify()
        for rows, n1, n2 in GUARD_TN:
            res.append(ops.gemm_atb_bf16(P(A[:rows, :n1].to(BF16)), P(B[:rows, :n2].to(BF16))).cpu())
        G.verify()
    return res


def test_gemms_stay_inside_their_buffers_and_read_nothing_unset(dev):
    """Inputs, outputs and workspaces inside guard bands under both fill bytes: every band intact, every result the
    same bits under 0x00 and 0xFF and equal to the CPU's — an empty K slice wrote its zero slab (under 0xFF an unwritten
    one is NaN), no row of A past the end and no slab was read unset."""
    from guarded import FILLS
    A, B = tn_inputs()
    want = []
    for a, w, b, y in _guard_nt_cases(dev):
        e = nt_expected(a, w, b, y)
        want += [e["biased"], e["relu_bf16"], e["masked"]]
    want += [tn_exact(A, B, rows, n1, n2) for rows, n1, n2 in GUARD_TN]
    runs = [_guarded_run(dev, fill) for fill in FILLS]
    assert len(runs[0]) == len(runs[1]) == len(want)
    for i, (r0, r1, e) in enumerate(zip(runs[0], runs[1], want)):
        assert not differ(r0, r1, bitwise=True), f"result {i} differs between fills {FILLS}: {differ(r0, r1, bitwise=True)}"
        d = differ(r0, e, bitwise=e.dtype == BF16)
        assert not d, f"result {i}: {d}"


if __name__ == "__main__":
    _child(sys.argv[1])
