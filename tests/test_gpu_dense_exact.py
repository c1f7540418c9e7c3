"""The fp32 and split-plane training GEMMs (csrc/train.hip, the split launchers of csrc/edge_mlp_split.hip and the two-plane
A^T.B of csrc/gemm_bf16.hip) and the row ops beside them, held to an fp64 CPU product PER ELEMENT at every dispatch
boundary.  A failure says how many elements differ and where the first one is (`differ`).

Method.  The oracle models nothing about summation order.  Three input families:

E1  operands and bias are integers in [-8, 8].  Every product is an integer of magnitude <= 64, every partial sum, in any
    order, an integer <= 64 K + 8 < 2^24 (asserted per case): no fp32 addition rounds, on the fp32 FMA, the fp32 MFMA or the
    plane products alike (an integer <= 8 is exact in one bf16 / fp16 plane), so the result EQUALS the fp64 product.
E2  (split paths) one operand is p + q 2^-8, p, q integers in [-4, 4], the other integers in [-4, 4]; both ways round.
    The integer operand is exact in its first plane, so every plane product that split_mma.h drops (a1 b2, a2 b1, a2 b2 of
    mma6_bf16; a1 b1 of MDNO_MMA3_F16) has a zero factor; every kept one is a multiple of the unit 2^-8 and the sum of the
    magnitudes of ALL kept products stays below 2^24 units: exact again.  The premise is checked on the CPU from the planes
    themselves (split3 / split2h of split_layout.h restated with torch casts): planes add up to the operand, each is a
    multiple of the unit, K max sum_p |a_p| max sum_p |w_p| (+ |bias|) < 2^24 units (for A^T.B, whose 4097 rows that
    product of maxima would miss by 0.4 %, the largest element of (sum_p |a_p|)^T (sum_p |b_p|) itself).  What the planes show: p + q 2^-8 has at
    most 11 significant bits, so it fills the first and second bf16 plane but never the third, and fits the fp16 hi plane
    alone.  Hence
E3  the same construction with the deeper planes in use: for fp16, p + q 2^-12 (15 bits: hi and lo plane; K <= 224 keeps
    224 . 16388 . 4 < 2^24); for bf16, p + q 2^-9 + r 2^-18 with p, q, r in {-1, 0, 1} against an operand in {-1, 0, 1}
    (three planes; only K = 32 keeps 32 . 262657 < 2^24).
    For split-f16, E2 / E3 rows of A and of W are multiplied by their own power of two, exponent in [-20, 20]
    (mdno_gemm_atb_split_f16: columns).  f16_row_scale brings every row back to [2^13, 2^14) and the epilogue undoes both
    scales, all powers of two: still exact.  These cases carry no bias — an integer plus a product scaled by 2^-40 is not an
    fp32 number.
G   Gaussian operands, one case per kernel: every element within c 2^-24 (sum |a||w| + |b|) of fp64 on the same fp32
    operands, c = 2 (n + 2) + s, n = contraction length + slice count.  (n + 2) 2^-24 is the any-order worst case of an fp32
    sum, doubled for an adder that truncates (as in test_gpu_gemm_pp.py).  s is the split's own term from split_layout.h:
    0 for fp32; three bf16 planes hold 24 bits and the dropped a1 b2 + a2 b1 + a2 b2 is below 2^-25 relative: s = 1; two
    fp16 planes represent each operand to 2^-23 (2 + 2 units of 2^-24 for the pair) and drop a1 b1 <= 2^-24: s = 5, taken
    as 6.  The worst error / bound per kernel is printed.

Every dispatch rule is restated below as a pure function and `test_case_lists_reach_every_dispatch_branch` asserts, without a
GPU, that the case lists reach every branch: a moved threshold fails there instead of silently un-testing a kernel.

Element-wise and row ops are compared with torch bit for bit (one IEEE multiply or a copy per element).

Largest error / bound measured on an MI355X: see `test_gaussian_within_the_any_order_bound_per_element`."""
import pytest
import torch

gpu = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16
LIMIT = 2 ** 24

ROWS_FEW = [1, 127, 128, 129, 257]
LIN_MFMA = dict(n=[128, 256], k=[32, 64, 96], rows=ROWS_FEW)
LIN_GENERIC = dict(n=[127, 129], k=[6, 31, 33], rows=ROWS_FEW)
LIN_MISALIGNED = (257, 128, 64)                      # (rows, n, k): tiles, but handed over 4 bytes into a buffer
BF16_N = [128, 1920, 2048, 2176]
BF16_ROWS = [1, 127, 128, 129, 255, 256, 257, 513]
BF16_K = [32, 64, 512]
# split-f16: rows at every edge of the padded row count (256) and of the kernel choice, per N
F16_ROWS = {128: [1],
            1024: [767, 768, 769, 1023, 1024, 1025, 1792, 1793, 2047, 2048, 2049, 4095, 4096, 4097],
            4096: [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]}
F16_K = [32, 64, 96, 128, 160, 192, 224]             # K / 32 stages: 1, then below / at / above both ring depths (3 and 6)
F16_GROUPS = {"wm1": [(128, 1), (1024, 768)], "wm2": [(4096, 1), (4096, 256), (1024, 769), (1024, 1024)],
              "wm4": [(4096, 257), (1024, 2048), (1024, 4096)], "big": [(1024, 4097), (4096, 1025)]}
ATB_MFMA = dict(widths=[(128, 128), (256, 128)], rows=[1, 31, 32, 33, 511, 512, 513, 1025])
ATB_GENERIC = dict(widths=[(100, 130), (7, 9)], rows=[1, 33, 513])
ATB_MISALIGNED = (513, 128, 128)
SMALLN_ROWS = [1, 127, 128, 129, 384, 385, 640, 641]
ATB_SMALLN = dict(n1=[1, 128, 255, 256, 257], n2=[1, 6, 8], rows=SMALLN_ROWS)
ATB_F16 = dict(widths=[(256, 256), (512, 256)], rows=[1, 31, 32, 33, 128, 129, 385, 513, 4097])
COLSUM_N = [1, 4, 7, 1020, 1024, 1028]
ELT_N = [1, 3, 4, 5, 64, 100]
ELT_ROWS = [1, 2, 255, 257]
TRANSPOSE = [(1, 1), (1, 33), (33, 1), (31, 32), (32, 32), (33, 65)]


@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ================================================================================================ dispatch rules, restated
def linear_f32_kernel(n, k, aligned=True):
    """mdno_linear_fwd."""
    return "mfma" if n % 128 == 0 and k % 32 == 0 and aligned else "generic"


def linear_mfma_main_loop_trips(k):
    return k // 32 - 1


def split_tiles(n, k, aligned=True):
    """What ops.linear asks before it takes a split kernel (split_linear_supported and the alignment of a, w)."""
    return k % 32 == 0 and n % 128 == 0 and aligned


def split_bf16_tile_rows(N):
    """split_linear: 256-row tiles for a wide N, 128-row tiles below."""
    return 256 if N >= 2048 else 128


def split_f16_kernel(N, rows):
    """launch_split_f16_gemm and launch_split_f16_gemm_small on the padded row count."""
    rows_pad = -(-rows // 256) * 256
    if (N // 128) * (rows_pad // 256) > 128:
        return "big"
    col_tiles = N // 64
    if col_tiles * (rows_pad // 128) >= 256:
        return "wm4"
    if col_tiles * (rows_pad // 64) >= 256:
        return "wm2"
    return "wm1"


def split_f16_ring(kernel):
    return 3 if kernel == "big" else 6


def atb_f32_kernel(n1, n2, aligned=True):
    """mdno_gemm_atb."""
    if n1 % 128 == 0 and n2 % 128 == 0 and aligned:
        return "mfma"
    return "smalln" if n2 <= 8 else "generic"


def atb_f32_slice_rows(rows, kernel):
    """Live rows of every slice: 16 slices rounded up to 32 rows, or 128 slices (small n / column sums)."""
    if kernel == "smalln":
        count, per = 128, -(-rows // 128)
    else:
        count, per = 16, -(-(-(-rows // 16)) // 32) * 32
    return [max(0, min(rows, z * per + per) - z * per) for z in range(count)]


def colsum_kernel(n, aligned=True):
    return "vec4" if n % 4 == 0 and aligned else "scalar"


def relu_bwd_kernel(n, aligned=True):
    return "vec4" if n % 4 == 0 and aligned else "scalar"


def atb_f16_slices(rows, n1, n2):
    """carve_atb_f16: a third of tn_slices (gemm_bf16.hip), at least one."""
    tiles = (n1 // 256) * (n2 // 256)
    sl = max(1, min(32, 256 // tiles))
    sl = min(sl, (rows + 127) // 128)
    while -(-rows // sl) * max(n1, n2) * 2 >= 2 ** 31:
        sl += 1
    return (sl + 2) // 3


def f16_cases():
    return [(N, rows) for N, rr in F16_ROWS.items() for rows in rr]


def test_case_lists_reach_every_dispatch_branch():
    """Host only.  Every branch named in the module docstring has a case, and the groups sit where the rules put them."""
    # mdno_linear_fwd
    assert {linear_f32_kernel(n, k) for n in LIN_MFMA["n"] for k in LIN_MFMA["k"]} == {"mfma"}
    assert {linear_f32_kernel(n, k) for n in LIN_GENERIC["n"] for k in LIN_GENERIC["k"]} == {"generic"}
    assert 0 in {linear_mfma_main_loop_trips(k) for k in LIN_MFMA["k"]} and max(map(linear_mfma_main_loop_trips, LIN_MFMA["k"])) >= 2
    rows, n, k = LIN_MISALIGNED
    assert linear_f32_kernel(n, k) == "mfma" and linear_f32_kernel(n, k, aligned=False) == "generic"
    assert split_tiles(n, k) and not split_tiles(n, k, aligned=False)
    for r in (1, 127, 128, 129):                     # one live row, one dead row, a full tile, one row into the next
        assert r in LIN_MFMA["rows"]
    # split_linear
    assert all(split_tiles(N, k) for N in BF16_N for k in BF16_K)
    assert [split_bf16_tile_rows(N) for N in BF16_N] == [128, 128, 256, 256]
    assert min(N for N in BF16_N if split_bf16_tile_rows(N) == 256) == 2048         # the threshold itself
    for edge in (128, 256):
        assert {edge - 1, edge, edge + 1} <= set(BF16_ROWS)
    assert 1 in BF16_ROWS and 513 in BF16_ROWS
    # split_linear_f16
    for name, group in F16_GROUPS.items():
        for N, r in group:
            assert split_f16_kernel(N, r) == name, (name, N, r, split_f16_kernel(N, r))
            assert (N, r) in f16_cases()
    assert {split_f16_kernel(N, r) for N, r in f16_cases()} == {"wm1", "wm2", "wm4", "big"}
    assert all(split_tiles(N, k) for N in F16_ROWS for k in F16_K)
    # every change of kernel along the rows has both neighbours in the list
    for N, rr in F16_ROWS.items():
        for r in range(1, max(rr)):
            if split_f16_kernel(N, r) != split_f16_kernel(N, r + 1):
                assert r in rr and r + 1 in rr, (N, r)
    rings = {split_f16_ring(split_f16_kernel(N, r)) for N, r in f16_cases()}
    assert rings == {3, 6}
    for ring in rings:
        assert {ring - 1, ring, ring + 1} <= {k // 32 for k in F16_K}
    assert 1 in {k // 32 for k in F16_K}
    # mdno_gemm_atb
    assert {atb_f32_kernel(*w) for w in ATB_MFMA["widths"]} == {"mfma"}
    assert {atb_f32_kernel(*w) for w in ATB_GENERIC["widths"]} == {"generic"}
    assert {atb_f32_kernel(n1, n2) for n1 in ATB_SMALLN["n1"] for n2 in ATB_SMALLN["n2"]} == {"smalln"}
    assert atb_f32_kernel(*ATB_MISALIGNED[1:], aligned=False) == "generic"
    empties = {r: atb_f32_slice_rows(r, "mfma").count(0) for r in ATB_MFMA["rows"]}
    assert empties[1] == 15 and empties[511] == 0 and empties[512] == 0 and empties[513] == 7 and empties[1025] == 5
    assert all(sum(atb_f32_slice_rows(r, kk)) == r for r in ATB_MFMA["rows"] + SMALLN_ROWS for kk in ("mfma", "smalln"))
    unroll = {r: max(atb_f32_slice_rows(r, "smalln")) for r in SMALLN_ROWS}
    assert unroll[384] == 3 and unroll[385] == 4 and unroll[640] == 5 and unroll[641] == 6       # the 4-row unroll and its tail
    assert atb_f32_slice_rows(1, "smalln").count(0) == 127
    # mdno_gemm_atb_split_f16
    assert {atb_f16_slices(r, *w) for w in ATB_F16["widths"] for r in ATB_F16["rows"]} == {1, 2, 11}
    # column sums, ReLU masks
    assert {colsum_kernel(n) for n in COLSUM_N} == {"vec4", "scalar"} and colsum_kernel(1024, aligned=False) == "scalar"
    assert {relu_bwd_kernel(n) for n in ELT_N} == {"vec4", "scalar"} and relu_bwd_kernel(64, aligned=False) == "scalar"


# ================================================================================================ inputs
def draw(g, kind, *shape):
    """(fp32 tensor, its unit).  Every value is an integer multiple of the unit."""
    ri = lambda lim: torch.randint(-lim, lim + 1, shape, generator=g).float()
    if kind == "int8":
        return ri(8), 1.0
    if kind == "int4":
        return ri(4), 1.0
    if kind == "tern":
        return ri(1), 1.0
    if kind == "m8":                                 # E2: two bf16 planes, one fp16 plane
        return ri(4) + ri(4) * 2.0 ** -8, 2.0 ** -8
    if kind == "m12":                                # E3 for fp16: hi and lo plane
        return ri(4) + ri(4) * 2.0 ** -12, 2.0 ** -12
    if kind == "m18":                                # E3 for bf16: three planes
        return ri(1) + ri(1) * 2.0 ** -9 + ri(1) * 2.0 ** -18, 2.0 ** -18
    raise KeyError(kind)


FAMILIES = {  # name: (kind of a, kind of w)
    "E1": ("int8", "int8"), "E2a": ("m8", "int4"), "E2w": ("int4", "m8"),
    "E3a_bf16": ("m18", "tern"), "E3w_bf16": ("tern", "m18"), "E3a_f16": ("m12", "int4"), "E3w_f16": ("int4", "m12")}


def pow2(g, n):
    return torch.ldexp(torch.ones(n), torch.randint(-20, 21, (n,), generator=g))


def misaligned(t):
    """The same values as a contiguous view that starts 4 bytes into its buffer."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ================================================================================================ the premise, from the planes
def planes_bf16(x):
    """split3 (split_layout.h)."""
    h = x.to(BF16).float()
    r1 = x - h
    m = r1.to(BF16).float()
    return [h, m, (r1 - m).to(BF16).float()]


def f16_scale(x, dim):
    """f16_row_scale of the largest magnitude along `dim` (kept): 2^(13 - exponent), 1 for an all-zero line."""
    mx = x.abs().amax(dim, keepdim=True)
    assert bool((mx == 0).logical_or(mx >= 2.0 ** -126).all())
    _, e = torch.frexp(mx)                           # mx = m 2^e, m in [0.5, 1): the IEEE exponent is e - 1
    return torch.where(mx == 0, torch.ones_like(mx), torch.ldexp(torch.ones_like(mx), (14 - e).clamp(-126, 126)))


def planes_f16(x, dim):
    """split2h (split_layout.h) of the scaled operand, the lo plane with its 2^11 taken out again; and the scale."""
    s = f16_scale(x, dim)
    xs = x * s
    assert torch.equal(xs.double(), x.double() * s.double())
    h = xs.to(F16).float()
    lo = ((xs - h) * 2048.0).to(F16).float()
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(lo).all())
    return [h, lo / 2048.0], s, xs


def check_premise(a, w, ua, uw, K, split, dim=1, a_line=None, w_line=None, bias=None):
    """Exactness of the kept plane products, from the planes.  a, w: the operands as the kernel gets them, contraction
    along `dim`; ua, uw their units; a_line, w_line the powers of two their lines (rows; columns for A^T.B) were multiplied
    by.  Returns which planes of a and of w are in use."""
    used, mags = [], []
    for x, u, line in ((a, ua, a_line), (w, uw, w_line)):
        if split == "bf16":
            pl, unit, total = planes_bf16(x), torch.full((), u), x
        elif split == "f16":
            pl, s, total = planes_f16(x, dim)
            unit = u * s * (line if line is not None else 1.0)
        else:
            pl, unit, total = [x], torch.full((), u), x
        assert torch.equal(sum(p.double() for p in pl), total.double()), "the planes do not add up to the operand"
        mag = torch.zeros_like(x, dtype=torch.float64)
        for p in pl:
            q = p.double() / unit.double()
            assert torch.equal(q, q.round()), "a plane is no multiple of the unit"
            mag += q.abs()
        used.append([bool(p.any()) for p in pl])
        mags.append(mag)
    if split in ("bf16", "f16"):
        dropped = [(i, j) for i in range(len(used[0])) for j in range(len(used[1])) if i + j > (2 if split == "bf16" else 1)]
        assert not any(used[0][i] and used[1][j] for i, j in dropped), "a dropped plane product is not zero"
    b = 0.0 if bias is None else float(bias.abs().max()) / (ua * uw)
    assert b == round(b)
    if dim == 0:                                     # A^T.B: the sum itself, per element (4097 rows need it)
        total = float((mags[0].T @ mags[1]).max())
    else:
        total = K * float(mags[0].max()) * float(mags[1].max())
    assert total + b < LIMIT, (K, total, b)
    return used


def representable(want64):
    assert torch.equal(want64.float().double(), want64), "the exact result is no fp32 number"
    return want64.float()


# ================================================================================================ comparison
def differ(got, want, bitwise=False):
    """"" where got equals want (bit for bit, or by value: +0 == -0, NaN differs from everything); otherwise how many
    elements differ and the first of them."""
    want = want.to(got.device)
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"got {got.dtype} {tuple(got.shape)}, want {want.dtype} {tuple(want.shape)}"
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)) if bitwise else (got != want)
    n = int(bad.sum())
    if n == 0:
        return ""
    i = tuple(bad.nonzero()[0].tolist())
    return f"{n} of {bad.numel()} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


def linear_exact(a, w, b):
    """The reference of every E case of a linear: the fp64 product (+ bias), as an fp32 tensor it must be equal to."""
    y = a.double() @ w.double().T
    return y if b is None else y + b.double()


def check_linear_table(dev, mode, a, w, b, rows_list, n_list, what, combos=((True, False), (False, True), (True, True), (False, False))):
    """ops.linear on a[:rows], w[:n] for the whole table against ONE fp64 product of the largest shape."""
    from molecular_dynamics_neural_operator_amd import ops
    plain = representable(linear_exact(a, w, None)).to(dev)
    biased = representable(linear_exact(a, w, b)).to(dev) if b is not None else None
    ad, wd, bd = a.to(dev), w.to(dev), (b.to(dev) if b is not None else None)
    for n in n_list:
        for rows in rows_list:
            for with_bias, relu in combos:
                if with_bias and b is None:
                    continue
                want = (biased if with_bias else plain)[:rows, :n]
                got = ops.linear(ad[:rows], wd[:n], bd[:n] if with_bias else None, relu=relu, gemm_mode=mode)
                d = differ(got, want.relu() if relu else want)
                assert not d, f"{what} {mode} rows={rows} n={n} k={a.shape[1]} bias={with_bias} relu={relu}: {d}"


# ================================================================================================ 1. ops.linear, fp32
@gpu
@pytest.mark.parametrize("k", LIN_MFMA["k"] + LIN_GENERIC["k"])
def test_linear_f32_equals_the_integer_product(dev, k):
    """E1 through mdno_linear_fwd: the MFMA kernel (k = 32: no trip of its main loop) and the one-thread-per-element kernel,
    with and without bias and ReLU, 1 .. 129 live rows in the last tile."""
    table = LIN_MFMA if k in LIN_MFMA["k"] else LIN_GENERIC
    g = torch.Generator().manual_seed(100 + k)
    (a, _), (w, _), (b, _) = draw(g, "int8", max(table["rows"]), k), draw(g, "int8", max(table["n"]), k), draw(g, "int8", max(table["n"]))
    check_premise(a, w, 1.0, 1.0, k, "none", bias=b)
    check_linear_table(dev, "f32", a, w, b, table["rows"], table["n"], "E1")


def _misaligned_linear_inputs():
    rows, n, k = LIN_MISALIGNED
    g = torch.Generator().manual_seed(7)
    (a, _), (w, _), (b, _) = draw(g, "int8", rows, k), draw(g, "int8", n, k), draw(g, "int8", n)
    check_premise(a, w, 1.0, 1.0, k, "none", bias=b)
    return a, w, b, representable(linear_exact(a, w, b))


@gpu
@pytest.mark.parametrize("mode", ["f32", "split_bf16", "split_f16"])
@pytest.mark.parametrize("which", ["a", "w"])
def test_linear_takes_the_fp32_kernel_for_a_misaligned_view(dev, mode, which):
    """A tiling shape whose a (or w) starts 4 bytes into its buffer: every mode falls to the one-thread-per-element fp32
    kernel, as ops.linear documents (the split entry points and the MFMA kernel need 16-byte operands), and E1 is exact."""
    from molecular_dynamics_neural_operator_amd import ops
    a, w, b, want = _misaligned_linear_inputs()
    ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
    if which == "a":
        ad = misaligned(ad)
    else:
        wd = misaligned(wd)
    d = differ(ops.linear(ad, wd, bd, relu=False, gemm_mode=mode), want)
    assert not d, f"{mode}, {which} misaligned: {d}"
    d = differ(ops.linear(ad, wd, bd, relu=True, gemm_mode=mode), want.relu())
    assert not d, f"{mode}, {which} misaligned, relu: {d}"


# ================================================================================================ 2. ops.linear, three bf16 planes
def bf16_families(k):
    return ["E1", "E2a", "E2w"] + (["E3a_bf16", "E3w_bf16"] if k == 32 else [])


@gpu
@pytest.mark.parametrize("k", BF16_K)
def test_linear_split_bf16_equals_the_exact_product(dev, k):
    """mdno_linear_split_fwd: 128-row tiles (N = 128, 1920) and 256-row tiles (N = 2048, 2176), rows 1 .. 513, E1, E2 both ways
    round and — at k = 32 — E3, whose operand fills all three planes."""
    seen = [set(), set()]
    for fi, fam in enumerate(bf16_families(k)):
        g = torch.Generator().manual_seed(2000 + 10 * k + fi)
        (a, ua), (w, uw) = draw(g, FAMILIES[fam][0], max(BF16_ROWS), k), draw(g, FAMILIES[fam][1], max(BF16_N), k)
        b = draw(g, "int8", max(BF16_N))[0]
        used = check_premise(a, w, ua, uw, k, "bf16", bias=b)
        for s, u in zip(seen, used):
            s.update(i for i, x in enumerate(u) if x)
        if fam.startswith("E2"):
            assert used[fam == "E2w"][:2] == [True, True]
        if fam.startswith("E3"):
            assert used[fam == "E3w_bf16"] == [True, True, True]
        check_linear_table(dev, "split_bf16", a, w, b, BF16_ROWS, BF16_N, fam, combos=((True, True), (False, False)))
    assert seen[0] == seen[1] == ({0, 1, 2} if k == 32 else {0, 1})


# ================================================================================================ 3. ops.linear, two fp16 planes
@gpu
@pytest.mark.parametrize("k", F16_K)
def test_linear_split_f16_equals_the_exact_product(dev, k):
    """mdno_linear_split_f16_fwd: the few-rows kernel at WM = 1, 2, 4 and the 256-row kernel, rows at every pad edge and at
    every change of kernel, the K loop 1 stage long and below / at / above both ring depths; fp32 output with and without
    ReLU.  E1 with bias; E2 and E3 with every row of A and of W times its own power of two."""
    for fi, fam in enumerate(["E1", "E2a", "E2w", "E3a_f16", "E3w_f16"]):
        g = torch.Generator().manual_seed(3000 + 10 * k + fi)
        rows_max = max(max(r) for r in F16_ROWS.values())
        (a, ua), (w, uw) = draw(g, FAMILIES[fam][0], rows_max, k), draw(g, FAMILIES[fam][1], max(F16_ROWS), k)
        if fam == "E1":
            b, sa, sw = draw(g, "int8", max(F16_ROWS))[0], None, None
        else:
            b, sa, sw = None, pow2(g, rows_max)[:, None], pow2(g, max(F16_ROWS))[:, None]
            a, w = a * sa, w * sw
        used = check_premise(a, w, ua, uw, k, "f16", a_line=sa, w_line=sw, bias=b)
        if fam.startswith("E3"):
            assert used[fam == "E3w_f16"] == [True, True]
        for N, rows_list in F16_ROWS.items():
            check_linear_table(dev, "split_f16", a[:max(rows_list)], w[:N], b[:N] if b is not None else None, rows_list, [N], fam,
                               combos=((True, True), (False, False), (False, True)))


# ================================================================================================ 4. ops.gemm_atb, fp32
def atb_exact(a, b, rows, n1, n2):
    return representable(a[:rows, :n1].double().T @ b[:rows, :n2].double())


def check_atb(dev, mode, a, b, rows, n1, n2, what, misalign=False):
    from molecular_dynamics_neural_operator_amd import ops
    ad, bd = a[:rows, :n1].contiguous().to(dev), b[:rows, :n2].contiguous().to(dev)
    if misalign:
        ad = misaligned(ad)
    got = ops.gemm_atb(ad, bd, gemm_mode=mode)
    d = differ(got, atb_exact(a, b, rows, n1, n2))
    assert not d, f"{what} {mode} rows={rows} ({n1}, {n2}): {d}"
    d = differ(ops.gemm_atb(ad, bd, gemm_mode=mode), got, bitwise=True)
    assert not d, f"{what} {mode} rows={rows} ({n1}, {n2}): the second call differs: {d}"


def atb_e1_inputs(seed, rows, n1, n2):
    g = torch.Generator().manual_seed(seed)
    (a, _), (b, _) = draw(g, "int8", rows, n1), draw(g, "int8", rows, n2)
    assert 64 * rows < LIMIT
    return a, b


@gpu
def test_gemm_atb_f32_mfma_and_generic_equal_the_integer_product(dev):
    """mdno_gemm_atb, 16 slices of whole 32-row steps: 15 empty slices at 1 row, 7 at 513, 5 at 1025, none at 511 and 512 — an
    empty slice must write its zero partial.  MFMA kernel, the one-thread-per-element kernel at widths that tile nothing,
    and at a tiling width whose A starts 4 bytes into its buffer.  Two calls give the same bits."""
    a, b = atb_e1_inputs(41, 1025, 256, 130)
    for n1, n2 in ATB_MFMA["widths"]:
        for rows in ATB_MFMA["rows"]:
            check_atb(dev, "f32", a, b, rows, n1, n2, "E1")
    for n1, n2 in ATB_GENERIC["widths"]:
        for rows in ATB_GENERIC["rows"]:
            check_atb(dev, "f32", a, b, rows, n1, n2, "E1")
    check_atb(dev, "f32", a, b, *ATB_MISALIGNED, "E1 misaligned", misalign=True)


@gpu
@pytest.mark.parametrize("n2", ATB_SMALLN["n2"])
def test_gemm_atb_f32_few_columns_equals_the_integer_product(dev, n2):
    """The thread-per-column-of-A kernel (n2 <= 8), 128 slices: 127 of them empty at 1 row, the 4-row unroll first entered at
    385 rows, entered with a tail at 641; n1 of 1, one block, one block + 1 and - 1."""
    a, b = atb_e1_inputs(42 + n2, max(SMALLN_ROWS), max(ATB_SMALLN["n1"]), n2)
    for n1 in ATB_SMALLN["n1"]:
        for rows in ATB_SMALLN["rows"]:
            check_atb(dev, "f32", a, b, rows, n1, n2, "E1")


# ================================================================================================ 5. ops.gemm_atb, two fp16 planes
@gpu
@pytest.mark.parametrize("n1,n2", ATB_F16["widths"])
def test_gemm_atb_split_f16_equals_the_exact_product(dev, n1, n2):
    """mdno_gemm_atb_split_f16 at 1, 2 and 11 K slices: E1; E2 and E3 both ways round with every column of A and of B times
    its own power of two; one column of A and one of B all zero (scale 1, a zero row / column of the result)."""
    from molecular_dynamics_neural_operator_amd import _lib
    lib = _lib.load()
    rows_max = max(ATB_F16["rows"])
    for fi, fam in enumerate(["E1", "E2a", "E2w", "E3a_f16", "E3w_f16"]):
        g = torch.Generator().manual_seed(5000 + n1 + fi)
        (a, ua), (b, ub) = draw(g, FAMILIES[fam][0], rows_max, n1), draw(g, FAMILIES[fam][1], rows_max, n2)
        sa = sb = None
        if fam != "E1":
            sa, sb = pow2(g, n1)[None, :], pow2(g, n2)[None, :]
            a, b = a * sa, b * sb
        a[:, 3] = 0.0
        b[:, 5] = 0.0
        for rows in ATB_F16["rows"]:
            if fam.startswith("E3") and rows > 224:
                continue                             # (rows . 16388 . 4 would pass 2^24 units)
            assert lib.mdno_gemm_atb_split_f16_supported(rows, n1, n2)
            used = check_premise(a[:rows], b[:rows], ua, ub, rows, "f16", dim=0, a_line=sa, w_line=sb)
            if fam.startswith("E3") and rows >= 31:
                assert used[fam == "E3w_f16"] == [True, True]
            check_atb(dev, "split_f16", a, b, rows, n1, n2, fam)


@gpu
def test_gemm_atb_split_f16_takes_the_fp32_kernel_for_a_misaligned_view(dev):
    a, b = atb_e1_inputs(43, 513, 256, 256)
    check_atb(dev, "split_f16", a, b, 513, 256, 256, "E1 misaligned", misalign=True)


# ================================================================================================ 6. column sums
@gpu
def test_colsum_equals_the_integer_sum(dev):
    """Both kernels (four columns per thread with 16-byte loads; one column per thread) at widths of 1, one quad, no whole
    quad, one block of quads - 1, exactly, + 1; the row list of the 128-slice split; and a quad width misaligned."""
    from molecular_dynamics_neural_operator_amd import ops
    a, _ = atb_e1_inputs(44, max(SMALLN_ROWS), max(COLSUM_N), 1)
    for n in COLSUM_N:
        for rows in SMALLN_ROWS:
            cut = a[:rows, :n].contiguous()
            want = representable(cut.double().sum(0))
            d = differ(ops.colsum(cut.to(dev)), want)
            assert not d, f"{colsum_kernel(n)} rows={rows} n={n}: {d}"
            if n == 1024:
                d = differ(ops.colsum(misaligned(cut.to(dev))), want)
                assert not d, f"misaligned rows={rows} n={n}: {d}"


# ================================================================================================ 7. accumulate = 1
@gpu
def test_accumulate_adds_the_exact_product_to_what_is_there(dev):
    """mdno_gemm_atb (MFMA, generic, few columns), mdno_colsum (both kernels) and mdno_gemm_atb_split_f16 with accumulate = 1,
    called as ops calls them: C preset to integers must come back as C0 + the exact product."""
    from molecular_dynamics_neural_operator_amd import _lib
    from molecular_dynamics_neural_operator_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    ws = lambda nbytes: torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(45)
    for rows, n1, n2 in [(513, 128, 128), (513, 100, 130), (385, 257, 6)]:
        a, b = atb_e1_inputs(46 + n2, rows, n1, n2)
        c0 = draw(g, "int8", n1, n2)[0]
        ad, bd, c = a.to(dev), b.to(dev), c0.to(dev)
        w = ws(lib.mdno_reduce_workspace_bytes(n1, n2))
        check(lib.mdno_gemm_atb(ptr(ad), ptr(bd), rows, n1, n2, ptr(c), 1, ptr(w), w.numel(), stream_ptr(dev)), "mdno_gemm_atb")
        d = differ(c, representable(c0.double() + a.double().T @ b.double()))
        assert not d, f"mdno_gemm_atb {atb_f32_kernel(n1, n2)} accumulate: {d}"
    for rows, n in [(385, 1024), (385, 7)]:
        a, _ = atb_e1_inputs(47 + n, rows, n, 1)
        c0 = draw(g, "int8", n)[0]
        ad, c = a.to(dev), c0.to(dev)
        w = ws(lib.mdno_reduce_workspace_bytes(n, 1))
        check(lib.mdno_colsum(ptr(ad), rows, n, ptr(c), 1, ptr(w), w.numel(), stream_ptr(dev)), "mdno_colsum")
        d = differ(c, representable(c0.double() + a.double().sum(0)))
        assert not d, f"mdno_colsum {colsum_kernel(n)} accumulate: {d}"
    rows, n1, n2 = 385, 256, 256
    a, b = atb_e1_inputs(48, rows, n1, n2)
    c0 = draw(g, "int8", n1, n2)[0]
    ad, bd, c = a.to(dev), b.to(dev), c0.to(dev)
    assert lib.mdno_gemm_atb_split_f16_supported(rows, n1, n2)
    w = ws(lib.mdno_gemm_atb_split_f16_workspace_bytes(rows, n1, n2))
    check(lib.mdno_gemm_atb_split_f16(ptr(ad), ptr(bd), rows, n1, n2, ptr(c), 1, ptr(w), w.numel(), stream_ptr(dev)),
          "mdno_gemm_atb_split_f16")
    d = differ(c, representable(c0.double() + a.double().T @ b.double()))
    assert not d, f"mdno_gemm_atb_split_f16 accumulate: {d}"


# ================================================================================================ 8. Gaussian operands
def ratio(got, want64, bound):
    err = (got.double().cpu() - want64).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


G_LINEAR = [  # (kernel, mode, rows, n, k, s)
    ("f32 mfma", "f32", 257, 256, 96, 0), ("f32 generic", "f32", 129, 129, 33, 0),
    ("bf16 128-row", "split_bf16", 257, 1920, 512, 1), ("bf16 256-row", "split_bf16", 257, 2048, 512, 1),
    ("f16 wm1", "split_f16", 768, 1024, 224, 6), ("f16 wm2", "split_f16", 1024, 1024, 224, 6),
    ("f16 wm4", "split_f16", 257, 4096, 224, 6), ("f16 big", "split_f16", 1025, 4096, 128, 6)]
G_ATB = [  # (kernel, mode, rows, n1, n2, s)
    ("f32 mfma", "f32", 1025, 256, 128, 0), ("f32 generic", "f32", 513, 100, 130, 0), ("f32 few columns", "f32", 641, 257, 6, 0),
    ("f16", "split_f16", 4097, 512, 256, 6)]


def test_gaussian_cases_sit_on_the_kernels_they_name():
    for name, mode, rows, n, k, _ in G_LINEAR:
        assert split_tiles(n, k) == (mode != "f32" or "mfma" in name)
        if mode == "f32":
            assert name == "f32 " + linear_f32_kernel(n, k)
        elif mode == "split_bf16":
            assert name == f"bf16 {split_bf16_tile_rows(n)}-row"
        else:
            assert name == "f16 " + split_f16_kernel(n, rows)
    assert [atb_f32_kernel(n1, n2) for _, m, _, n1, n2, _ in G_ATB if m == "f32"] == ["mfma", "generic", "smalln"]


@gpu
def test_gaussian_within_the_any_order_bound_per_element(dev):
    """One Gaussian case per kernel, every element within (2 (n + 2) + s) 2^-24 (sum |a||w| + |b|) of fp64 on the same fp32
    operands; the worst error / bound is printed.  Measured on an MI355X — linear: f32 mfma 0.020, f32 generic 0.057,
    bf16 128-row 0.0045, bf16 256-row 0.0043, f16 wm1 0.0043, wm2 0.0044, wm4 0.0044, big 0.0090; A^T.B: f32 mfma 4.1e-4,
    generic 8.2e-4, few columns 3.7e-4, f16 4.2e-5; colsum: vec4 2.5e-4, scalar 4.7e-5."""
    from molecular_dynamics_neural_operator_amd import ops
    worst = {}
    for name, mode, rows, n, k, s in G_LINEAR:
        g = torch.Generator().manual_seed(rows + n + k)
        a, w, b = torch.randn(rows, k, generator=g), torch.randn(n, k, generator=g), torch.randn(n, generator=g)
        want = a.double() @ w.double().T + b.double()
        bound = (2 * (k + 1 + 2) + s) * 2.0 ** -24 * (a.double().abs() @ w.double().abs().T + b.double().abs())
        worst["linear " + name] = ratio(ops.linear(a.to(dev), w.to(dev), b.to(dev), gemm_mode=mode), want, bound)
    for name, mode, rows, n1, n2, s in G_ATB:
        g = torch.Generator().manual_seed(rows + n1 + n2)
        a, b = torch.randn(rows, n1, generator=g), torch.randn(rows, n2, generator=g)
        want = a.double().T @ b.double()
        slices = atb_f16_slices(rows, n1, n2) if mode == "split_f16" else len(atb_f32_slice_rows(rows, atb_f32_kernel(n1, n2)))
        bound = (2 * (rows + slices + 2) + s) * 2.0 ** -24 * (a.double().abs().T @ b.double().abs())
        worst["atb " + name] = ratio(ops.gemm_atb(a.to(dev), b.to(dev), gemm_mode=mode), want, bound)
    for rows, n in [(641, 1024), (641, 7)]:
        a = torch.randn(rows, n, generator=torch.Generator().manual_seed(n))
        bound = 2 * (rows + 128 + 2) * 2.0 ** -24 * a.double().abs().sum(0)
        worst[f"colsum {colsum_kernel(n)}"] = ratio(ops.colsum(a.to(dev)), a.double().sum(0), bound)
    for name, r in worst.items():
        print(f"{name}: largest error / bound {r:.3g}")
    over = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not over, over


# ================================================================================================ 9. element-wise and row ops
def draw_y(g, rows, n):
    """-1, -0.0, +0.0, the smallest positive subnormal, 1."""
    vals = torch.tensor([0xBF800000 - 2 ** 32, 0x80000000 - 2 ** 32, 0, 1, 0x3F800000], dtype=torch.int64).to(torch.int32)
    return vals[torch.randint(0, 5, (rows, n), generator=g)].view(torch.float32)


def elementwise_inputs(rows, n):
    g = torch.Generator().manual_seed(9000 + 1000 * rows + n)
    y = draw_y(g, rows, n)
    keep = y.view(torch.int32) > 0                   # sign clear and not zero: the subnormal counts
    assert torch.equal(keep, y.double() > 0)
    return torch.randn(rows, n, generator=g), y, torch.randn(rows, generator=g), keep


@gpu
@pytest.mark.parametrize("rows", ELT_ROWS)
def test_relu_masks_and_row_scales_equal_torch_bit_for_bit(dev, rows):
    """relu_bwd with and without row_scale (both kernels, and the 16-byte one's shapes misaligned), relu_bwd2 against the two
    relu_bwd calls and against torch, relu_mask_bwd, scale_rows: where(y > 0, g . scale, +0) with y from
    {-1, -0.0, +0.0, the smallest subnormal, 1}; g finite."""
    from molecular_dynamics_neural_operator_amd import ops
    zero = torch.zeros(())
    for n in ELT_N:
        g, y, sc, keep = elementwise_inputs(rows, n)
        gd, yd, sd = g.to(dev), y.to(dev), sc.to(dev)
        want = torch.where(keep, g, zero)
        want_s = torch.where(keep, g * sc[:, None], zero)
        what = f"rows={rows} n={n}"
        d = differ(ops.relu_bwd(gd, yd), want, bitwise=True)
        assert not d, f"relu_bwd {what}: {d}"
        d = differ(ops.relu_bwd(gd, yd, sd), want_s, bitwise=True)
        assert not d, f"relu_bwd row_scale {what}: {d}"
        d = differ(ops.relu_mask_bwd(gd, yd), want, bitwise=True)
        assert not d, f"relu_mask_bwd {what}: {d}"
        d = differ(ops.scale_rows(gd, sd), g * sc[:, None], bitwise=True)
        assert not d, f"scale_rows {what}: {d}"
        if n % 4 == 0:
            d = differ(ops.relu_bwd(misaligned(gd), yd, sd), want_s, bitwise=True)
            assert not d, f"relu_bwd, g misaligned {what}: {d}"
            d = differ(ops.relu_bwd(gd, misaligned(yd), None), want, bitwise=True)
            assert not d, f"relu_bwd, y misaligned {what}: {d}"
            gz, gs = torch.empty_like(gd), torch.empty_like(gd)
            ops.relu_bwd2(gd, yd, sd, gz, gs)
            assert not differ(gz, ops.relu_bwd(gd, yd), bitwise=True) and not differ(gs, ops.relu_bwd(gd, yd, sd), bitwise=True)
            d = differ(gz, want, bitwise=True) or differ(gs, want_s, bitwise=True)
            assert not d, f"relu_bwd2 {what}: {d}"


@gpu
def test_relu_bwd2_refuses_operands_that_are_not_16_byte_aligned(dev):
    """mdno_relu_bwd2 reads and writes 16 bytes at a time: a misaligned g, y, gz or gs is MDNO_EINVAL before any launch (the
    outputs keep what they held)."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd._lib import EINVAL, MdnoError
    g, y, sc, _ = elementwise_inputs(2, 64)
    gd, yd, sd = g.to(dev), y.to(dev), sc.to(dev)
    for bad in range(4):
        gz, gs = torch.full_like(gd, 7.0), torch.full_like(gd, 7.0)
        args = [gd, yd, gz, gs]
        args[bad] = misaligned(args[bad])
        with pytest.raises(MdnoError, match=rf"code {EINVAL}\).*16-byte"):
            ops.relu_bwd2(args[0], args[1], sd, args[2], args[3])
        torch.cuda.synchronize()
        assert bool((args[2] == 7.0).all()) and bool((args[3] == 7.0).all())


@gpu
def test_transpose_and_row_moves_equal_torch_bit_for_bit(dev):
    """transpose at one element, one row, one column, a tile - 1, a tile, a tile + 1 in both directions; permute_rows
    (a gather: repeats allowed) and scatter_rows (its inverse on a permutation) at the element-wise widths and row counts."""
    from molecular_dynamics_neural_operator_amd import ops
    g = torch.Generator().manual_seed(77)
    for r, c in TRANSPOSE:
        a = torch.randn(r, c, generator=g)
        d = differ(ops.transpose(a.to(dev)), a.T.contiguous(), bitwise=True)
        assert not d, f"transpose ({r}, {c}): {d}"
    for rows in ELT_ROWS:
        for n in ELT_N:
            x = torch.randn(rows + 3, n, generator=g)
            pick = torch.randint(0, rows + 3, (rows,), generator=g).to(torch.int32)
            d = differ(ops.permute_rows(x.to(dev), pick.to(dev), rows), x[pick.long()], bitwise=True)
            assert not d, f"permute_rows rows={rows} n={n}: {d}"
            perm = torch.randperm(rows, generator=g).to(torch.int32)
            want = torch.empty(rows, n)
            want[perm.long()] = x[:rows]
            d = differ(ops.scatter_rows(x[:rows].contiguous().to(dev), perm.to(dev), rows), want, bitwise=True)
            assert not d, f"scatter_rows rows={rows} n={n}: {d}"
