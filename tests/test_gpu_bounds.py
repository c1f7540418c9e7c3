"""No byte outside, none read unset: every buffer the kernels are given lies between two guard bands (tests/guarded.py).

Each GPU case runs its operation twice, once per fill byte (0x00 and 0xFF: zeros, and fp32 / bf16 NaN / int32 -1),
and asserts
  1. the bands around every allocation the package made (outputs, workspaces) and around every input are intact,
  2. the valid extent of every output is bitwise the same under both fills (nothing that was never written is read),
  3. the result against the reference and tolerance the suite already uses for that op (fp64 torch for primitives:
     tests/test_gpu_training.py; `close` of tests/test_gpu_parity.py for graphs, the edge-MLP, convs and forwards; the
     oracle's train step and tests/bf16_replica.py for training; tests/test_gpu_forecast.py for scoring).
Shapes sit on and around the tile edges: 64-row node kernels, 128 / 256-row GEMM tiles, the 1,024-row threshold of the
edge-MLP workspace layout.  `gemm_atb` "split_f16" and `linear_bf16_masked` need multiples of 256, which the n / k list
{1, 3, 6, 64, 100, 128, 130, 384} does not hold: they run at 256.

COVERAGE maps every entry point of include/mdno.h that can write caller memory to the case that runs it under guard;
the CPU test below fails for an entry point that has neither a case nor an exemption, and the last GPU test compares
the table with what the guard recorded."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded
from guarded import FILLS, Guard, GuardError

gpu = pytest.mark.gpu

# entry point -> the test that runs it inside a Guard
COVERAGE = {
    "mdno_radius_graph_csr": "test_radius_graph",
    "mdno_radius_graph_csr_ws": "test_radius_graph, test_radius_graph_cell_list",
    "mdno_coo_to_csr": "test_coo_to_csr_and_by_source",
    "mdno_csr_by_source": "test_coo_to_csr_and_by_source",
    "mdno_edge_mlp_fwd": "test_edge_mlp",
    "mdno_nnconv_fwd": "test_conv_ops",
    "mdno_node_prologue_fwd": "test_train_step",
    "mdno_fc_out_fwd": "test_train_step",
    "mdno_kernelnn_fwd": "test_forward",
    "mdno_kernelnn_fallback_counts": "test_forward",
    "mdno_rollout": "test_rollout_one_shot_entry",
    "mdno_rollout_plan_create": "test_rollout",
    "mdno_rollout_plan_run": "test_rollout",
    "mdno_rollout_plan_fallback_counts": "test_rollout",
    "mdno_adam_step": "test_adam",
    "mdno_pack_tensors": "test_pack_unpack_abutting_slots",
    "mdno_unpack_tensors": "test_pack_unpack_abutting_slots",
    "mdno_linear_fwd": "test_dense_fp32",
    "mdno_linear_split_fwd": "test_dense_fp32",
    "mdno_linear_split_f16_fwd": "test_dense_fp32",
    "mdno_gemm_atb": "test_dense_fp32",
    "mdno_gemm_atb_split_f16": "test_dense_fp32",
    "mdno_colsum": "test_dense_fp32",
    "mdno_relu_bwd2": "test_dense_fp32",
    "mdno_relu_bwd": "test_dense_fp32",
    "mdno_transpose": "test_dense_fp32",
    "mdno_inv_degree": "test_dense_fp32",
    "mdno_scale_rows": "test_dense_fp32",
    "mdno_relu_mask_bwd": "test_dense_fp32",
    "mdno_permute_rows": "test_dense_fp32",
    "mdno_scatter_rows": "test_dense_fp32",
    "mdno_cast_bf16": "test_dense_bf16",
    "mdno_linear_smallk_bf16_fwd": "test_dense_bf16",
    "mdno_linear_bf16_fwd": "test_dense_bf16",
    "mdno_linear_bf16_masked": "test_dense_bf16",
    "mdno_gemm_atb_bf16": "test_dense_bf16",
    "mdno_relu_bwd_bf16": "test_dense_bf16",
    "mdno_colsum_bf16": "test_dense_bf16",
    "mdno_colsum_atb_bf16": "test_dense_bf16",
    "mdno_nnconv_bwd_x": "test_conv_ops",
    "mdno_nnconv_bwd_root": "test_conv_ops",
    "mdno_nnconv_bwd_root_pair": "test_conv_ops",
    "mdno_nnconv_bwd_we": "test_conv_ops",
    "mdno_nnconv_bwd_we_colsum": "test_conv_ops",
    "mdno_nnconv_bf16w_fwd": "test_conv_ops",
    "mdno_nnconv_bwd_x_bf16w": "test_conv_ops",
    "mdno_nnconv_bwd_we_bf16": "test_conv_ops",
    "mdno_nnconv_bwd_we_bf16_colsum": "test_conv_ops",
    "mdno_nnconv_chain_fwd": "test_conv_ops",
    "mdno_nnconv_chain_bwd": "test_conv_ops",
    "mdno_nnconv_chain_bf16w_fwd": "test_conv_ops",
    "mdno_nnconv_chain_bf16w_bwd": "test_conv_ops",
    "mdno_nnconv_msg_grad": "test_conv_ops",
    "mdno_nnconv_bwd_x_edges": "test_conv_ops",
    "mdno_nnconv_bwd_we_edges": "test_conv_ops",
    "mdno_collate_samples": "test_device_trajectory_batch",
    "mdno_lploss_rel_fwd": "test_lploss",
    "mdno_lploss_rel_bwd": "test_lploss",
    "mdno_node_prologue_bwd": "test_train_step",
    "mdno_fc_out_bwd": "test_train_step",
    "mdno_forecast_score": "test_scoring",
    "mdno_contact_maps": "test_scoring",
}
# entry points with a non-const pointer that write no caller buffer on the device
EXEMPT = {
    "mdno_rollout_plan_steps_per_launch": "reads a field of the host plan handle",
    "mdno_rollout_plan_destroy": "frees the host plan handle; no device buffer is written",
    "mdno_rollout_plan_timer_attach": "measurement aid: allocates HIP events inside the plan handle",
    "mdno_rollout_plan_timer_read": "writes two host scalars from the plan's events",
    "mdno_rollout_plan_timer_detach": "measurement aid: frees the plan's events",
}
# entry point with a workspace_bytes parameter -> the function that states its size
WORKSPACE_OF = {
    "mdno_radius_graph_csr_ws": "mdno_radius_graph_workspace_bytes",
    "mdno_coo_to_csr": "mdno_coo_to_csr_workspace_bytes",
    "mdno_csr_by_source": "mdno_coo_to_csr_workspace_bytes",
    "mdno_edge_mlp_fwd": "mdno_edge_mlp_workspace_bytes",
    "mdno_kernelnn_fwd": "mdno_kernelnn_workspace_bytes",
    "mdno_rollout": "mdno_rollout_workspace_bytes",
    "mdno_rollout_plan_create": "mdno_rollout_workspace_bytes",
    "mdno_linear_split_fwd": "mdno_linear_split_workspace_bytes",
    "mdno_linear_split_f16_fwd": "mdno_linear_split_f16_workspace_bytes",
    "mdno_gemm_atb": "mdno_reduce_workspace_bytes",
    "mdno_gemm_atb_split_f16": "mdno_gemm_atb_split_f16_workspace_bytes",
    "mdno_colsum": "mdno_reduce_workspace_bytes",
    "mdno_nnconv_bwd_root_pair": "mdno_nnconv_bwd_root_pair_workspace_bytes",
    "mdno_nnconv_bwd_root": "mdno_nnconv_bwd_root_workspace_bytes",
    "mdno_linear_bf16_fwd": "mdno_linear_bf16_workspace_bytes",
    "mdno_linear_bf16_masked": "mdno_linear_bf16_workspace_bytes",
    "mdno_gemm_atb_bf16": "mdno_gemm_atb_bf16_workspace_bytes",
    "mdno_nnconv_bwd_we_colsum": "mdno_nnconv_bwd_we_colsum_workspace_bytes",
    "mdno_nnconv_bwd_we_bf16_colsum": "mdno_nnconv_bwd_we_bf16_colsum_workspace_bytes",
    "mdno_colsum_bf16": "mdno_colsum_bf16_workspace_bytes",
    "mdno_colsum_atb_bf16": "mdno_colsum_atb_bf16_workspace_bytes",
    "mdno_node_prologue_bwd": "mdno_node_prologue_bwd_workspace_bytes",
    "mdno_fc_out_bwd": "mdno_fc_out_bwd_workspace_bytes",
    "mdno_forecast_score": "mdno_forecast_score_workspace_bytes",
}

RECORDED = set()        # entry points that ran inside a Guard in this process
RAN = set()             # GPU tests of this file that ran (the last test skips if a selection left some out)


# =============================================================================== CPU: the helper, the table
def test_guard_self_test_on_a_cpu_arena():
    """Plain host writes into memory the test owns: one byte past the payload names the trailing band at offset 0, one
    byte before it the leading band at its last offset; an untouched arena passes; zeros are zero under both fills."""
    for fill in FILLS:
        with Guard(fill, device_type="cpu", record_calls=False) as G:
            t = torch.empty((3, 5), dtype=torch.float32)
            z = torch.zeros(7, dtype=torch.int32)
            zl = torch.zeros_like(t, dtype=torch.bfloat16)
            f = torch.full((2, 2), 7.0)
            e = torch.empty_like(t)
            host = torch.empty(4, device="meta")                          # other device types pass through
            assert len(G.records) == 5 and host.device.type == "meta"
            assert t.is_contiguous() and e.shape == t.shape and t.data_ptr() % 64 == 0
            assert int(z.abs().sum()) == 0 and float(zl.float().abs().sum()) == 0.0 and bool((f == 7.0).all())
            assert bool((t.view(torch.uint8) == fill).all())
            if fill == 0xFF:
                assert bool(torch.isnan(t).all()) and int(torch.empty(2, dtype=torch.int32)[0]) == -1
            p = G.place(torch.arange(6.0).reshape(2, 3))
            assert torch.equal(p, torch.arange(6.0).reshape(2, 3))
            G.verify()                                                    # untouched: passes
            r = G.records[0]
            assert r.nbytes == 60 and r.offset == guarded.FRONT >= 64 * 1024 and r.trailing().numel() >= 1024 * 1024
            r.base[r.offset + r.nbytes] = fill ^ 0x5A
            with pytest.raises(GuardError, match=r"60 bytes at test_gpu_bounds.py:\d+ in test_guard_self_test.*trailing band "
                                                 r"overwritten, first bad offset 0 of \d+, 1 bad byte"):
                G.verify()
            r.base[r.offset + r.nbytes] = fill
            r.base[r.offset - 1] = fill ^ 0x5A
            with pytest.raises(GuardError, match=rf"leading band overwritten, first bad offset {guarded.FRONT - 1} of "
                                                 rf"{guarded.FRONT}, 1 bad byte"):
                G.verify()
            r.base[r.offset - 1] = fill
            G.verify()
    assert all(getattr(torch, n).__name__ == n for n in guarded.PATCHED)


def test_every_writing_entry_point_has_a_case_or_an_exemption():
    decls = guarded.header_functions()
    from molecular_dynamics_neural_operator_amd import _lib
    assert set(decls) == set(_lib.SIGNATURES)
    writers = {n for n, p in decls.items() if guarded.writes_memory(p)}
    assert not set(COVERAGE) & set(EXEMPT)
    missing = writers - set(COVERAGE) - set(EXEMPT)
    assert not missing, f"entry points without a bounds case or an exemption: {sorted(missing)}"
    assert set(COVERAGE) <= writers and set(EXEMPT) <= writers, (set(COVERAGE) | set(EXEMPT)) - writers
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())
    tests = {k for k, v in globals().items() if k.startswith("test_") and callable(v)}
    for name, where in COVERAGE.items():
        assert {w.strip() for w in where.split(",")} <= tests, (name, where)
    with_ws = {n for n, p in decls.items() if any(q == "workspace_bytes" for _, q in p)}
    assert with_ws == set(WORKSPACE_OF) and all(v in decls for v in WORKSPACE_OF.values())
    print(f"{len(COVERAGE)} of {len(decls)} declared entry points run under guard; {len(EXEMPT)} exempt; "
          f"{len(decls) - len(writers)} write no caller memory")


# =============================================================================== GPU helpers
@pytest.fixture(scope="module")
def dev():
    from molecular_dynamics_neural_operator_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from oracle import graph_kernel_oracle
    return graph_kernel_oracle


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    if "gpu" in request.keywords and torch.cuda.is_available():
        RAN.add(request.node.originalname)


def rel_err(a, b):
    from test_gpu_training import rel_err as r
    return r(a, b)


def close(a, b, **kw):
    from test_gpu_parity import close as c
    return c(a, b, **kw)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _cpu(v):
    if torch.is_tensor(v):
        return v.detach().cpu().clone()
    if isinstance(v, dict):
        return {k: _cpu(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_cpu(x) for x in v]
    return v


def _flat(v, pre=""):
    if isinstance(v, dict):
        for k, x in v.items():
            yield from _flat(x, f"{pre}{k}.")
    elif isinstance(v, list):
        for i, x in enumerate(v):
            yield from _flat(x, f"{pre}{i}.")
    else:
        yield pre[:-1], v


def both_fills(run, **guard_kw):
    """run(G) -> the VALID extents of the outputs (tensors, nested in dicts / lists).  Runs it under each fill, checks
    the guards after each run, then that the two results have the same bits; returns the first (on the host)."""
    res = []
    for fill in FILLS:
        with Guard(fill, **guard_kw) as G:
            out = run(G)
            G.verify()
            res.append(_cpu(out))
            RECORDED.update(G.calls)
    a, b = dict(_flat(res[0])), dict(_flat(res[1]))
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert same_bits(a[k], b[k]), f"{k}: differs between fill 0x00 and fill 0xFF (reads memory nothing wrote)"
        else:
            assert a[k] == b[k], k
    return res[0]


ROWS = [1, 63, 64, 65, 127, 129, 255, 257, 1023, 1025]
NK = [1, 3, 6, 64, 100, 128, 130, 384]


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


# =============================================================================== dense primitives, fp32
@gpu
@pytest.mark.parametrize("rows", ROWS)
def test_dense_fp32(dev, rows):
    from molecular_dynamics_neural_operator_amd import ops
    g = _gen(1, rows)
    nk = [(1, 1), (3, 6), (6, 3), (64, 64), (100, 130), (130, 100), (128, 64), (384, 128), (128, 384), (64, 100)]
    lin_in = [(torch.randn(rows, k, generator=g), torch.randn(n, k, generator=g), torch.randn(n, generator=g)) for n, k in nk]
    atb_n = [(1, 1), (3, 6), (64, 64), (100, 130), (128, 384), (384, 1), (256, 256)]
    atb_in = [(torch.randn(rows, n1, generator=g), torch.randn(rows, n2, generator=g)) for n1, n2 in atb_n]
    # the 1 x 1 product is ONE sum over the rows: with signed terms it cancels (|sum| << sum |terms|) and the norm-relative
    # error of that single entry measures the cancellation, not the kernel; positive operands keep it a sum of like terms
    atb_in[0] = (atb_in[0][0].abs(), atb_in[0][1].abs())
    ew = {n: (torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g), torch.rand(rows, generator=g) + 0.1) for n in NK}
    perm = torch.randperm(rows, generator=g).to(torch.int32)
    deg = torch.randint(0, 5, (rows,), generator=g)
    deg[0] = 0 if rows > 1 else 3
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).to(torch.int32)

    def run(G):
        P = lambda t_: G.place(t_.to(dev))
        out = {}
        for i, (a, w, b) in enumerate(lin_in):
            A, Wt, B = P(a), P(w), P(b)
            for mode in ("f32", "split_bf16", "split_f16"):
                out[f"lin{i}.{mode}"] = ops.linear(A, Wt, B if i % 2 == 0 else None, relu=bool(i % 3 == 0), gemm_mode=mode)
        for i, (a, b) in enumerate(atb_in):
            A, B = P(a), P(b)
            out[f"atb{i}.f32"] = ops.gemm_atb(A, B)
            out[f"atb{i}.f16"] = ops.gemm_atb(A, B, gemm_mode="split_f16")
            out[f"colsum{i}"] = ops.colsum(A)
        for n, (gq, y, sc) in ew.items():
            Gq, Y, Sc = P(gq), P(y), P(sc)
            out[f"tr{n}"] = ops.transpose(Gq)
            out[f"rb{n}"] = ops.relu_bwd(Gq, Y)
            out[f"rbs{n}"] = ops.relu_bwd(Gq, Y, Sc)
            if n % 4 == 0:              # (mdno_relu_bwd2 takes n % 4 == 0 only and says so)
                gz, gs = torch.empty((rows, n), device=dev), torch.empty((rows, n), device=dev)
                ops.relu_bwd2(Gq, Y, Sc, gz, gs)
                out[f"rb2z{n}"], out[f"rb2s{n}"] = gz, gs
            out[f"scale{n}"] = ops.scale_rows(Gq, Sc)
            out[f"mask{n}"] = ops.relu_mask_bwd(Gq, Y)
            Pm = P(perm)
            out[f"perm{n}"] = ops.permute_rows(Gq, Pm, rows)
            out[f"scat{n}"] = ops.scatter_rows(Gq, Pm, rows)
        gr = ops.CSRGraph(P(row_ptr), None, None, None, 0)
        out["inv_mean"], out["inv_add"] = ops.inv_degree(gr, "mean"), ops.inv_degree(gr, "add")
        return out

    got = both_fills(run)
    for i, (a, w, b) in enumerate(lin_in):
        want = F.linear(a.double(), w.double(), b.double() if i % 2 == 0 else None)
        want = want.relu() if i % 3 == 0 else want
        for mode in ("f32", "split_bf16", "split_f16"):
            e = rel_err(got[f"lin{i}.{mode}"], want)
            print(f"linear rows={rows} (n,k)={nk[i]} {mode}: rel err {e:.2e}")
            assert e < 2e-6, (nk[i], mode, e)
    for i, (a, b) in enumerate(atb_in):
        want = a.double().t() @ b.double()
        assert rel_err(got[f"atb{i}.f32"], want) < 2e-6 and rel_err(got[f"atb{i}.f16"], want) < 2e-6, atb_n[i]
        assert rel_err(got[f"colsum{i}"], a.double().sum(0)) < 2e-6
    for n, (gq, y, sc) in ew.items():
        m = gq * (y > 0)
        assert torch.equal(got[f"tr{n}"], gq.t().contiguous())
        assert torch.equal(got[f"rb{n}"], m) and torch.equal(got[f"mask{n}"], m)
        torch.testing.assert_close(got[f"rbs{n}"], m * sc[:, None])
        if n % 4 == 0:
            assert torch.equal(got[f"rb2z{n}"], m) and torch.equal(got[f"rb2s{n}"], got[f"rbs{n}"])
        close(got[f"scale{n}"], gq.double() * sc.double()[:, None], name=f"scale_rows n={n}")
        assert torch.equal(got[f"perm{n}"], gq[perm.long()])
        want = torch.empty_like(gq)
        want[perm.long()] = gq
        assert torch.equal(got[f"scat{n}"], want)
    torch.testing.assert_close(got["inv_mean"], 1.0 / deg.clamp_min(1).float())
    assert torch.equal(got["inv_add"], torch.ones(rows))


# =============================================================================== dense primitives, bf16
@gpu
@pytest.mark.parametrize("rows", ROWS)
def test_dense_bf16(dev, rows):
    from molecular_dynamics_neural_operator_amd import ops
    g = _gen(2, rows)
    bf = lambda t_: t_.to(torch.bfloat16)
    lin_nk = [(128, 64), (384, 128), (128, 384), (256, 64), (256, 128)]
    lin_in = [(torch.randn(rows, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g),
               torch.randn(rows, n, generator=g)) for n, k in lin_nk]
    small_nk = [(64, 1), (64, 3), (128, 6), (384, 6), (8, 8)]
    small_in = [(torch.randn(rows, k, generator=g), torch.randn(n, k, generator=g), torch.randn(n, generator=g)) for n, k in small_nk]
    atb_n = [(128, 128), (128, 384), (384, 128)]
    atb_in = [(torch.randn(rows, n1, generator=g), torch.randn(rows, n2, generator=g)) for n1, n2 in atb_n]
    cs_in = {n: torch.randn(rows, n, generator=g) for n in (64, 128, 384)}
    kb_in = {kb: torch.randn(rows, kb, generator=g) * 10 for kb in (6, 8)}
    ew = {n: (torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g)) for n in (64, 100, 128, 384)}

    def run(G):
        P = lambda t_: G.place(t_.to(dev))
        out = {}
        for i, (a, w, b, y) in enumerate(lin_in):
            A, Wt, B, Y = P(bf(a)), P(w), P(b), P(bf(y))
            out[f"lin{i}.f32"] = ops.linear_bf16(A, Wt, B, relu=False, out_bf16=False)
            out[f"lin{i}.bf16"] = ops.linear_bf16(A, Wt, B, relu=True, out_bf16=True)
            out[f"masked{i}"] = ops.linear_bf16_relu_bwd(A, Wt, Y)
        for i, (a, w, b) in enumerate(small_in):
            out[f"small{i}"] = ops.linear_smallk_bf16(P(a), P(w), P(b), relu=bool(i % 2))
        for i, (a, b) in enumerate(atb_in):
            out[f"atb{i}"] = ops.gemm_atb_bf16(P(bf(a)), P(bf(b)))
        for n, a in cs_in.items():
            A = P(bf(a))
            out[f"cast{n}"] = ops.cast_bf16(P(a))
            out[f"colsum{n}"] = ops.colsum_bf16(A)
            for kb, b in kb_in.items():
                out[f"csatb{n}.{kb}"] = list(ops.colsum_atb_bf16(A, P(b)))
        for n, (gq, y) in ew.items():
            Gq, Y = P(gq), P(bf(y))
            out[f"rb{n}.f32"] = ops.relu_bwd_bf16(Gq, Y, out_bf16=False)
            out[f"rb{n}.bf16"] = ops.relu_bwd_bf16(Gq, Y, out_bf16=True)
        return out

    got = both_fills(run)
    for i, (a, w, b, y) in enumerate(lin_in):
        prod = F.linear(bf(a).double(), bf(w).double())
        assert rel_err(got[f"lin{i}.f32"], prod + b.double()) < 3e-6, lin_nk[i]
        assert got[f"lin{i}.bf16"].dtype == torch.bfloat16
        assert rel_err(got[f"lin{i}.bf16"].float(), (prod + b.double()).relu()) < 4e-3, lin_nk[i]      # one bf16 rounding
        assert rel_err(got[f"masked{i}"].float(), prod * (bf(y).double() > 0)) < 4e-3, lin_nk[i]        # one bf16 rounding
    for i, (a, w, b) in enumerate(small_in):
        want = F.linear(a.double(), w.double(), b.double())
        want = want.relu() if i % 2 else want
        assert got[f"small{i}"].dtype == torch.bfloat16 and rel_err(got[f"small{i}"].float(), want) < 4e-3, small_nk[i]
    for i, (a, b) in enumerate(atb_in):
        assert rel_err(got[f"atb{i}"], bf(a).double().t() @ bf(b).double()) < 3e-6, atb_n[i]
    for n, a in cs_in.items():
        assert torch.equal(got[f"cast{n}"], bf(a))
        assert rel_err(got[f"colsum{n}"], bf(a).double().sum(0)) < 3e-6
        for kb, b in kb_in.items():
            cs, atb = got[f"csatb{n}.{kb}"]
            assert rel_err(cs, bf(a).double().sum(0)) < 2e-6 and rel_err(atb, bf(a).double().t() @ b.double()) < 2e-6, (n, kb)
    for n, (gq, y) in ew.items():
        m = gq * (bf(y).float() > 0)
        assert torch.equal(got[f"rb{n}.f32"], m) and torch.equal(got[f"rb{n}.bf16"], bf(m))


# =============================================================================== graphs
@gpu
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("N", [1, 28, 97, 504])
def test_radius_graph(dev, O, M, N):
    """edge_cap exactly E, E - 1 (truncated and flagged: nothing at index cap) and the minimum (R rows); the entry
    without a workspace gives the same graph."""
    from molecular_dynamics_neural_operator_amd import _lib, ops, synthetic as syn
    thr = 8.0
    frames = np.stack([syn.box_frame(N, seed=40 + m) for m in range(M)]).astype(np.float32)
    want = np.concatenate([O.radius_graph_coo(frames[m], thr) + m * N for m in range(M)], axis=1)
    E, R = want.shape[1], M * N
    pos = torch.from_numpy(frames).reshape(R, 3)

    def run(G):
        p = G.place(pos.to(dev))
        out = {}
        for tag, cap in (("tight", E), ("short", max(E - 1, R)), ("min", R)):
            g = ops.radius_graph(p, N, thr, edge_cap=cap)
            e = min(E, cap)
            assert g.src.numel() == cap and g.edge_count() == e
            out[tag] = dict(row_ptr=g.row_ptr, src=g.src[:e], dst=g.dst[:e], ne=g.num_edges, status=g.status)
        lib = _lib.load()
        row_ptr = torch.empty(R + 1, dtype=torch.int32, device=dev)
        src, dst = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
        ne, st = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.mdno_radius_graph_csr(p.data_ptr(), M, N, thr, row_ptr.data_ptr(), src.data_ptr(), dst.data_ptr(), E,
                                             ne.data_ptr(), st.data_ptr(), _lib.stream_ptr(dev)), "mdno_radius_graph_csr")
        out["plain"] = dict(row_ptr=row_ptr, src=src, dst=dst, ne=ne, status=st)
        return out

    got = both_fills(run)
    for tag in ("tight", "plain"):
        g = got[tag]
        assert int(g["status"]) == 0 and int(g["ne"]) == E
        assert np.array_equal(torch.stack([g["dst"], g["src"]]).numpy(), want), tag
        assert int(g["row_ptr"][-1]) == E
    for tag, cap in (("short", max(E - 1, R)), ("min", R)):
        g = got[tag]
        assert int(g["ne"]) == min(E, cap) and bool(int(g["status"]) & _lib.STATUS_EDGE_OVERFLOW) == (cap < E)
        assert np.array_equal(torch.stack([g["dst"], g["src"]]).numpy(), want[:, :min(E, cap)]), tag
        assert int(g["row_ptr"].max()) == min(E, cap)


@gpu
def test_radius_graph_cell_list(dev, O):
    """N >= 8,192: the cell list's workspace between bands; the same graph as the pair tests, and — with a workspace one
    byte short — the documented fallback to the pair tests, bit for bit."""
    from molecular_dynamics_neural_operator_amd import ops, synthetic as syn
    N = 8200
    pos = torch.from_numpy(syn.box_frame(N, seed=3).astype(np.float32))
    cap = N * 700

    def graph(G, **kw):
        g = ops.radius_graph(G.place(pos.to(dev)), N, 8.0, edge_cap=cap, **kw)
        e = g.edge_count()
        return dict(row_ptr=g.row_ptr, src=g.src[:e], dst=g.dst[:e], status=g.status)

    cell = both_fills(lambda G: graph(G, cell_list=True))
    brute = both_fills(lambda G: graph(G, cell_list=False))
    assert int(cell["status"]) == 0 and cell["src"].numel() >= N
    want = O.radius_graph_coo(pos.numpy(), 8.0)                     # scipy fp64 pair tests on the same frame
    assert np.array_equal(torch.stack([cell["dst"], cell["src"]]).numpy(), want)
    assert all(torch.equal(cell[k], brute[k]) for k in cell)
    seen = []

    def short(G):
        out = graph(G, cell_list=True)
        seen.extend(G.undersized)
        return out
    fell_back = both_fills(short, undersize={"mdno_radius_graph_csr_ws": WORKSPACE_OF["mdno_radius_graph_csr_ws"]})
    assert len(seen) == 2 and seen[0][1] > 0
    assert all(torch.equal(fell_back[k], brute[k]) for k in cell)


def _odd_graphs():
    """(name, nodes, edge_index): no edge, one edge, odd counts with empty rows, a hub target and source, duplicates."""
    g = torch.Generator().manual_seed(12)
    out = [("E0", 5, torch.zeros((2, 0), dtype=torch.long)), ("E1", 1, torch.zeros((2, 1), dtype=torch.long)),
           ("E1far", 65, torch.tensor([[64], [0]]))]
    for n, E in ((7, 33), (65, 777), (129, 3001)):
        ei = torch.randint(0, n, (2, E), generator=g)
        ei[1, : E // 3] = n - 1                      # hub target
        ei[0, E // 3: E // 2] = 0                    # hub source
        ei[:, -5:] = ei[:, :5]                       # duplicates
        ei[1, ei[1] == 1] = 2                        # node 1: no in-edge
        ei[0, ei[0] == 3] = 2                        # node 3: no out-edge
        out.append((f"n{n}E{E}", n, ei))
    return out


@gpu
@pytest.mark.parametrize("name,n,ei", _odd_graphs(), ids=[c[0] for c in _odd_graphs()])
def test_coo_to_csr_and_by_source(dev, name, n, ei):
    from molecular_dynamics_neural_operator_amd import ops
    E = ei.shape[1]

    def run(G):
        g = ops.coo_to_csr(G.place(ei.to(dev)), n)
        out = dict(row_ptr=g.row_ptr, src=g.src[:E], dst=g.dst[:E], perm=g.perm[:E], ne=g.num_edges, status=g.status)
        if E:
            s = ops.source_sorted(g, n)
            out["by_src"] = dict(row_ptr=s.row_ptr, nbr=s.src[:E], rowid=s.dst[:E], perm=s.perm[:E])
        return out

    got = both_fills(run)
    order = torch.sort(ei[1], stable=True).indices
    assert int(got["ne"]) == E and int(got["status"]) == 0
    assert torch.equal(got["perm"].long(), order) and torch.equal(got["src"].long(), ei[0][order])
    assert torch.equal(got["dst"].long(), ei[1][order])
    counts = torch.bincount(ei[1], minlength=n)
    assert torch.equal(got["row_ptr"].long(), torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]))
    if E:
        s_src, s_dst = ei[0][order], ei[1][order]
        order2 = torch.sort(s_src, stable=True).indices
        b = got["by_src"]
        assert torch.equal(b["perm"].long(), order2) and torch.equal(b["nbr"].long(), s_dst[order2])
        assert torch.equal(b["rowid"].long(), s_src[order2])
        c2 = torch.bincount(s_src, minlength=n)
        assert torch.equal(b["row_ptr"].long(), torch.cat([torch.zeros(1, dtype=torch.long), c2.cumsum(0)]))


# =============================================================================== edge MLP
def _edge_mlp_cases():
    """ker_width x out_dim x capacity x (E < cap, E == cap) x GEMM mode x edge source, every value of each in a covering
    set (a full product is 432 fp64 oracles); the 1,024-row layout threshold sits between capacities 1,000 and 1,025."""
    out = []
    kws, caps, modes = [100, 128, 256, 1024], [1000, 1025, 2049], ["f32", "split_bf16", "split_f16"]
    i = 0
    for kw in kws:
        for od in (9, kw, 4096):
            for full in (False, True):
                out.append(dict(kw=kw, od=od, cap=caps[i % 3], full=full, mode=modes[(i // 2) % 3], src=("attr", "pos")[(i + i // 6) % 2]))
                i += 1
    for j, cap in enumerate(caps):                 # the tiled shapes at every capacity in every split mode
        for mode in modes:
            out.append(dict(kw=1024, od=4096, cap=cap, full=bool(j % 2), mode=mode, src="pos"))
            out.append(dict(kw=128, od=4096, cap=cap, full=not bool(j % 2), mode=mode, src="attr"))
    seen, uniq = set(), []
    for c in out:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


@gpu
@pytest.mark.parametrize("c", _edge_mlp_cases(), ids=lambda c: "k{kw}o{od}cap{cap}{f}-{mode}-{src}".format(f="full" if c["full"] else "part", **c))
def test_edge_mlp(dev, O, c):
    from molecular_dynamics_neural_operator_amd import ops
    kw, od, cap = c["kw"], c["od"], c["cap"]
    E = cap if c["full"] else cap - 37
    g = _gen(3, kw, od, cap, E)
    R = 77
    pos = torch.randn(R, 3, generator=g) * 5
    src, dst = torch.randint(0, R, (E,), generator=g).to(torch.int32), torch.randint(0, R, (E,), generator=g).to(torch.int32)
    perm = torch.randperm(E, generator=g).to(torch.int32)
    ea = torch.cat([pos[src.long()], pos[dst.long()]], dim=1) if c["src"] == "pos" else torch.randn(E, 6, generator=g) * 5
    torch.manual_seed(kw + od)
    lins = [torch.nn.Linear(6, kw), torch.nn.Linear(kw, kw), torch.nn.Linear(kw, od)]
    sd = {}
    for j, lin in zip((0, 2, 4), lins):
        sd[f"layers.{j}.weight"], sd[f"layers.{j}.bias"] = lin.weight.data, lin.bias.data
    attrs = ea if c["src"] == "pos" else ea[perm.long()]
    want = O.edge_mlp(attrs, sd, "")

    def run(G):
        P = lambda t_: G.place(t_.to(dev))
        w = [P(sd[f"layers.{j}.{n}"]) for j in (0, 2, 4) for n in ("weight", "bias")]
        ne = P(torch.full((1,), E, dtype=torch.int32))
        if c["src"] == "pos":          # src / dst hold exactly the E valid entries: a read at E reads the band
            gr = ops.CSRGraph(None, P(src), P(dst), ne, cap, None, None)
            return ops.edge_mlp(w, 6, kw, od, gr, edge_pos=P(pos), gemm_mode=c["mode"])[:E]
        gr = ops.CSRGraph(None, None, None, ne, cap, P(perm), None)
        return ops.edge_mlp(w, 6, kw, od, gr, edge_attr=P(ea), gemm_mode=c["mode"])[:E]

    got = both_fills(run)
    close(got, want, name=str(c))


# =============================================================================== convolution
def _conv_graph(R, gen):
    """A hub (a third of the edges into one row), an isolated node, duplicates; R = 1: self-loops only."""
    E = 1 if R == 1 else 6 * R + 1
    ei = torch.randint(0, R, (2, E), generator=gen)
    if R > 2:
        ei[1, : E // 3] = R - 1
        ei[:, -3:] = ei[:, :3]
        ei[1, ei[1] == 1] = 0
        ei[0, ei[0] == 1] = 0                        # node 1: isolated
    return ei


@gpu
@pytest.mark.parametrize("R", [1, 63, 65, 129])
def test_conv_ops(dev, O, R):
    """nnconv add / mean / max (+ the zero-edge graph), the chain forward and backward with fp32 and bf16 W_e,
    nnconv_bwd_x, nnconv_bwd_we with and without its column sums at L <= 16 and L > 16, bwd_root / bwd_root_pair and
    the per-edge message gradients, at 64 x 64 and at 5 x 3 channels."""
    from molecular_dynamics_neural_operator_amd import ops
    gen = _gen(4, R)
    ei = _conv_graph(R, gen)
    E = ei.shape[1]
    depth = 2
    L = 2 * depth
    x = torch.randn(R, 64, generator=gen)
    w_e = torch.randn(E, 4096, generator=gen) * 0.05
    r1, r2 = [torch.randn(64, 64, generator=gen) * 0.2 for _ in range(2)]
    b1, b2 = [torch.randn(64, generator=gen) for _ in range(2)]
    gy = torch.randn(R, 64, generator=gen)
    XL = {l: (torch.randn(l, R, 64, generator=gen), torch.randn(l, R, 64, generator=gen) * 0.3) for l in (1, 12, 18)}
    xs, ws, rs, gsm = (torch.randn(R, 5, generator=gen), torch.randn(E, 15, generator=gen), torch.randn(5, 3, generator=gen),
                       torch.randn(R, 3, generator=gen))
    order = torch.sort(ei[1], stable=True).indices

    def run(G):
        P = lambda t_: G.place(t_.to(dev))
        out = {}
        g = ops.coo_to_csr(P(ei), R)
        by_src = ops.source_sorted(g, R)
        X, Wc, R1, R2, B1, B2, Gy = P(x), P(w_e[order]), P(r1), P(r2), P(b1), P(b2), P(gy)
        Wb = P(w_e[order].to(torch.bfloat16))
        for aggr in ("add", "mean", "max"):
            out[f"y.{aggr}"] = ops.nnconv(X, g, Wc, R1, B1, aggr, relu=(aggr == "mean"))
        out["y.bf16w"] = ops.nnconv_bf16w(X, g, Wb, R1, B1, "mean", relu=True)
        g0 = ops.coo_to_csr(torch.zeros((2, 0), dtype=torch.long, device=dev), R)
        out["y.noedges"] = ops.nnconv(X, g0, Wc[:0], R1, B1, "mean")
        inv = ops.inv_degree(g, "mean")
        gz, gs = ops.relu_bwd(Gy, out["y.mean"]), ops.relu_bwd(Gy, out["y.mean"], inv)
        out["gx"] = ops.nnconv_bwd_x(gz, gs, by_src, Wc, R1)
        out["gx.bf16w"] = ops.nnconv_bwd_x_bf16w(gz, gs, by_src, Wb, R1)
        out["d_root"], out["d_bias"] = ops.nnconv_bwd_root(X, gz)
        for l, (xl, gl) in XL.items():
            Xl, Gl = P(xl), P(gl)
            out[f"dwe{l}"] = ops.nnconv_bwd_we(Xl, Gl, g)
            out[f"dwe{l}.cs"] = list(ops.nnconv_bwd_we(Xl, Gl, g, with_colsum=True))
            out[f"dweb{l}"] = ops.nnconv_bwd_we_bf16(Xl, Gl, g)
            out[f"dweb{l}.cs"] = list(ops.nnconv_bwd_we_bf16(Xl, Gl, g, with_colsum=True))
        out["pair"] = list(ops.nnconv_bwd_root_pair(P(XL[12][0]), P(XL[12][1])))
        for tag, W in (("f32", Wc), ("bf16", Wb)):
            Xs = torch.zeros((L + 1, R, 64), device=dev)
            Xs[0].copy_(X)
            ops.nnconv_chain_fwd(Xs, g, W, R1, B1, R2, B2, depth)
            out[f"chain.{tag}.x"] = Xs
            out[f"chain.{tag}.bwd"] = list(ops.nnconv_chain_bwd(Gy, Xs, inv, by_src, W, R1, R2, depth))
        Xsm, Wsm, Rsm, Gsm = P(xs), P(ws[order]), P(rs), P(gsm)
        for aggr in ("add", "mean", "max"):
            gm = ops.nnconv_msg_grad(Xsm, g, Wsm, Gsm, aggr)
            out[f"gm.{aggr}"] = gm[:E]
            out[f"dx.{aggr}"] = ops.nnconv_bwd_x_edges(gm, Gsm, by_src, Wsm, Rsm, 5)
            out[f"dwes.{aggr}"] = ops.nnconv_bwd_we_edges(Xsm, gm, g)
        return out

    got = both_fills(run)
    d = lambda t_: t_.double()
    for aggr in ("add", "mean", "max"):
        want = O.nnconv_apply(d(x), ei, d(w_e), d(r1), d(b1), aggr)
        close(got[f"y.{aggr}"], want.relu() if aggr == "mean" else want, name=f"nnconv {aggr} R={R}")
    wb = w_e.to(torch.bfloat16)
    close(got["y.bf16w"], O.nnconv_apply(d(x), ei, d(wb), d(r1), d(b1), "mean").relu(), name="nnconv bf16w")
    close(got["y.noedges"], d(x) @ d(r1) + d(b1), name="nnconv without edges")
    # backward of relu(mean conv) against autograd in fp64 (tests/test_gpu_training.py: rel. L2 < 1e-5)
    x64, w64, r64, b64 = [t_.double().requires_grad_() for t_ in (x, w_e, r1, b1)]
    torch.relu(O.nnconv_apply(x64, ei, w64, r64, b64, "mean")).backward(d(gy))
    assert rel_err(got["gx"], x64.grad) < 1e-5 and rel_err(got["d_root"], r64.grad) < 1e-5
    assert rel_err(got["d_bias"], b64.grad) < 1e-5
    xb = x.double().requires_grad_()         # (the device took the ReLU mask from its fp32-weight forward: y.mean)
    O.nnconv_apply(xb, ei, d(wb), d(r1), d(b1), "mean").backward(d(gy) * (got["y.mean"] > 0).double())
    assert rel_err(got["gx.bf16w"], xb.grad) < 1e-5
    src, dst = ei[0][order], ei[1][order]
    for l, (xl, gl) in XL.items():
        want = torch.einsum("lei,leo->eio", d(xl)[:, src], d(gl)[:, dst]).reshape(E, 4096)
        mag = torch.einsum("lei,leo->eio", d(xl)[:, src].abs(), d(gl)[:, dst].abs()).reshape(E, 4096)
        for key, ulp in ((f"dwe{l}", 0.0), (f"dweb{l}", 2.0 ** -8)):
            for t_ in (got[key], got[key + ".cs"][0]):
                assert bool(((d(t_) - want).abs() <= want.abs() * ulp + mag * 2.0 ** -20).all()), (key, R)
            dw, cs = got[key + ".cs"]
            assert float((d(cs) - d(dw).sum(0)).abs().max()) <= 1e-5 * max(float(d(dw).abs().sum(0).max()), 1e-30), key
    xl, gl = XL[12]
    for k, sl in ((0, slice(0, 6)), (2, slice(6, 12))):
        xx, gg = d(xl[sl]).reshape(-1, 64), d(gl[sl]).reshape(-1, 64)
        assert rel_err(got["pair"][k], xx.t() @ gg) < 2e-6 and rel_err(got["pair"][k + 1], gg.sum(0)) < 2e-6
    for tag, W in (("f32", w_e), ("bf16", wb)):
        Xs, pre = [x.double().requires_grad_()], []
        for a in range(1, L + 1):
            pre.append(O.nnconv_apply(Xs[-1], ei, d(W), d(r1 if a <= depth else r2), d(b1 if a <= depth else b2), "mean"))
            pre[-1].retain_grad()
            Xs.append(torch.relu(pre[-1]))
        Xs[-1].backward(d(gy))
        close(got[f"chain.{tag}.x"], torch.stack([t_.detach() for t_ in Xs]), name=f"chain fwd {tag}")
        gz_ref = torch.stack([t_.grad for t_ in pre])          # gz[a-1] = dLoss / d(pre-activation of application a)
        inv_ref = 1.0 / torch.bincount(ei[1], minlength=R).clamp_min(1).double()
        gz_, gs_, g_in = got[f"chain.{tag}.bwd"]
        close(gz_, gz_ref, name=f"chain bwd gz {tag}")
        close(gs_, gz_ref * inv_ref[None, :, None], name=f"chain bwd gs {tag}")
        close(g_in, Xs[0].grad, name=f"chain bwd g_in {tag}")
    for aggr in ("add", "mean", "max"):
        xs64, ws64, rs64 = [t_.double().requires_grad_() for t_ in (xs, ws, rs)]
        O.nnconv_apply(xs64, ei, ws64, rs64, torch.zeros(3, dtype=torch.float64), aggr).backward(d(gsm))
        close(got[f"dx.{aggr}"], xs64.grad, name=f"dx edges {aggr}")
        # dLoss/dm_e: autograd through the aggregation of the messages alone (CSR edge order)
        msg = torch.einsum("ei,eio->eo", d(xs)[src], d(ws)[order].view(E, 5, 3)).requires_grad_()
        if aggr == "max":
            agg = torch.zeros(R, 3, dtype=torch.float64).index_reduce(0, dst, msg, "amax", include_self=False)
        else:
            agg = torch.zeros(R, 3, dtype=torch.float64).index_add(0, dst, msg)
            if aggr == "mean":
                agg = agg / torch.bincount(dst, minlength=R).clamp_min(1).double()[:, None]
        agg.backward(d(gsm))
        close(got[f"gm.{aggr}"], msg.grad, name=f"msg_grad {aggr}")
        close(got[f"dwes.{aggr}"], ws64.grad[order], name=f"d_we edges {aggr}")


# =============================================================================== whole forward
def _fwd_cases():
    out = []
    for i, N in enumerate([1, 28, 63, 65, 129]):
        for j, M in enumerate([1, 3]):
            for conv in ("materialized", "factored"):
                out.append(dict(N=N, M=M, conv=conv, k=(128, 1024)[(i + j) % 2], tight=bool((i + j + (conv == "factored")) % 2),
                                gemm=("split_f16", "split_bf16", "f32")[(i + j) % 3], width=64))
    out.append(dict(N=65, M=3, conv="materialized", k=100, tight=True, gemm="split_f16", width=24))     # off-tile: generic path
    out.append(dict(N=28, M=1, conv="materialized", k=100, tight=False, gemm="f32", width=24))
    return out


@gpu
@pytest.mark.parametrize("c", _fwd_cases(), ids=lambda c: "n{N}m{M}k{k}w{width}-{conv}-{gemm}-{t}".format(t="tight" if c["tight"] else "loose", **c))
def test_forward(dev, O, c):
    """ops.kernelnn_forward on its own radius graph (positions + CSR), materialized and forced factored — atom counts
    that are no multiple of 64 are the shape of the factored workspace's old size / carve disagreement — with and
    without the latent, edge capacity == E and loose."""
    from molecular_dynamics_neural_operator_amd import _lib, ops, synthetic as syn
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    N, M, W, thr = c["N"], c["M"], 4, 8.0
    sd = near_identity_state_dict(c["width"], c["k"], seed=N + M, kernel_gain=2e-2, feature_gain=0.2, kernel_to_coords=1.0)
    base = syn.jitter_window(syn.chain_frame(N, seed=N), W, seed=N)
    wins = syn.ensemble_windows(base, M, sigma=0.2, seed0=N)                          # [M,W,N,3]
    aa = torch.from_numpy(syn.amino_acids(N, seed=N))
    tm = torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3)))          # [W,M,N,3]
    refs = [O.construct_pairdata(wins[m], aa, thr) for m in range(M)]
    E = sum(r["edge_index"].shape[1] for r in refs)
    cap = E if c["tight"] else 2 * E + 100

    def run(G):
        pack = ops.ParamPack({k: G.place(v.to(dev)) for k, v in sd.items()}, 2, dev, gemm_mode=c["gemm"], conv_mode=c["conv"])
        frames = G.place(tm.to(dev))
        last = frames[W - 1].reshape(M * N, 3)
        ran = int(_lib.load().mdno_resolve_conv_mode(pack.ref, M, cap))
        assert ran == _lib.CONV_MODES[c["conv"]], "the case did not run the formulation its id names"
        out = {}
        for latent in (False, True):
            g = ops.radius_graph(last, N, thr, edge_cap=cap)
            counts = {}
            o, lat = ops.kernelnn_forward(pack, frames, G.place(aa.to(dev)), g, edge_pos=last, return_latent=latent,
                                          fallback_counts=counts)
            out[f"out{int(latent)}"] = o
            out["counts"] = counts
            if latent:
                out["latent"] = lat
            assert g.edge_count() == E
        return out

    got = both_fills(run)
    assert same_bits(got["out0"], got["out1"])
    from types import SimpleNamespace
    from test_gpu_model_shapes import _oracle_forward
    for m in range(M):
        r = refs[m]
        want, want_lat = _oracle_forward(sd, SimpleNamespace(x_position=r["x_position"], x_aminoacid=aa, edge_index=r["edge_index"],
                                                             edge_attr=r["edge_attr"]), 2)
        close(got["out1"][m * N:(m + 1) * N], want, name=f"forward member {m}")
        close(got["latent"][m * N:(m + 1) * N], want_lat, name=f"latent member {m}")


# =============================================================================== rollout
def _rollout_setup(N, M, W, k=128, seed=0):
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    sd = near_identity_state_dict(64, k, seed=seed + 1, kernel_gain=2e-2, feature_gain=0.2, kernel_to_coords=1.0)
    model = KernelNN(64, k, 2, 6, 7, 3, 20, 4)
    model.load_state_dict(sd)
    base = syn.jitter_window(syn.chain_frame(N, seed=seed), W, seed=seed)
    wins = syn.ensemble_windows(base, M, sigma=0.2, seed0=seed)
    aa = torch.from_numpy(syn.amino_acids(N, seed=seed))
    tm = torch.from_numpy(np.ascontiguousarray(wins.transpose(1, 0, 2, 3)))
    return sd, model, wins, aa, tm


def _oracle_rollout(O, sd, wins, aa, steps, thr=8.0):
    out = []
    for m in range(wins.shape[0]):
        fc = O.recursive_propagation(sd, 2, O.construct_pairdata(wins[m], aa, thr), steps, thr, hoist=True)
        out.append(np.stack([f["x_position"][-1].numpy() for f in fc]))
    return np.stack(out, axis=1)                   # [steps, M, N, 3]


@gpu
@pytest.mark.parametrize("N,M,steps,use_graph,conv", [(28, 1, 11, True, "materialized"), (28, 1, 11, False, "materialized"),
                                                      (65, 3, 3, True, "materialized"), (65, 3, 3, False, "factored"),
                                                      (1, 3, 2, True, "materialized")])
def test_rollout(dev, O, N, M, steps, use_graph, conv):
    """steps == max_steps: the last produced frame is the last row of the trajectory buffer.  N = 28 with 11 steps: the
    short-chain plan replays 8 per launch and finishes on the one-step graph."""
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    W = 3
    sd, model, wins, aa, tm = _rollout_setup(N, M, W, seed=N)
    model.eval().to(dev)
    model.conv_mode = conv

    def run(G):
        eng = RolloutEngine(model, M, N, W, 8.0, max_steps=steps, device=dev, use_graph=use_graph)
        traj = eng.run(G.place(tm.to(dev)), G.place(aa.to(dev)), steps)
        assert traj.data_ptr() + traj.numel() * 4 == eng.traj.data_ptr() + eng.traj.numel() * 4
        out = dict(traj=traj.clone(), edges=eng.edges_per_step.clone(), counts=eng.fallback_counts(), spl=eng.steps_per_launch)
        G.verify()
        eng.close()
        return out

    got = both_fills(run)
    if N == 28:
        assert got["spl"] == (8 if use_graph else 0)
    want = _oracle_rollout(O, sd, wins, aa, steps)
    close(got["traj"], want, name=f"rollout N={N} M={M}")


@gpu
def test_rollout_capacity_regrow(dev, O):
    """N = 260 without an edge capacity: fitted to the start window, outgrown when the untrained model pulls the cloud
    together, regrown (new workspace, new plan) and re-run."""
    from molecular_dynamics_neural_operator_amd import synthetic as syn
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    N, W, steps, thr = 260, 4, 4, 8.0
    torch.manual_seed(5)
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.eval().to(dev)
    win = syn.jitter_window(syn.chain_frame(N, seed=7), W, seed=7)
    aa = torch.from_numpy(syn.amino_acids(N, seed=7))

    def run(G):
        eng = RolloutEngine(model, 1, N, W, thr, max_steps=steps, device=dev)
        traj = eng.run(torch.from_numpy(win), aa, steps)
        assert eng.regrown
        out = dict(traj=traj.clone(), edges=eng.edges_per_step.clone())
        G.verify()
        eng.close()
        return out

    got = both_fills(run)
    close(got["traj"], _oracle_rollout(O, sd, win[None], aa, steps), name="regrown rollout")


@gpu
def test_grouped_rollout(dev, O):
    from molecular_dynamics_neural_operator_amd.rollout import GroupedRolloutEngine
    N, M, W, steps = 28, 3, 3, 5
    sd, model, wins, aa, tm = _rollout_setup(N, M, W, seed=9)
    model.eval().to(dev)

    def run(G):
        eng = GroupedRolloutEngine(model, M, N, W, 8.0, max_steps=steps, groups=2, device=dev)
        traj = eng.run(tm, aa, steps).clone()
        out = dict(traj=traj, edges=eng.edges_per_step.clone())
        G.verify()
        eng.close()
        return out

    got = both_fills(run)
    close(got["traj"], _oracle_rollout(O, sd, wins, aa, steps), name="grouped rollout")


@gpu
def test_rollout_one_shot_entry(dev, O):
    """mdno_rollout (no plan handle), graph replay and plain launches: frames W .. W+steps-1 of a buffer that ends there."""
    from molecular_dynamics_neural_operator_amd import _lib, ops
    N, M, W, steps = 28, 1, 3, 3
    sd, model, wins, aa, tm = _rollout_setup(N, M, W, seed=4)
    lib = _lib.load()

    def run(G):
        out = {}
        pack = ops.ParamPack({k: G.place(v.to(dev)) for k, v in sd.items()}, 2, dev, gemm_mode="split_f16")
        for use_graph in (1, 0):
            traj = torch.zeros((W + steps, M, N, 3), device=dev)
            traj[:W].copy_(tm.to(dev))
            cap = N * N
            nb = lib.mdno_rollout_workspace_bytes(pack.ref, M, N, cap)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            eps, status = torch.zeros(steps, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            aad = G.place(aa.to(dev))
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            _lib.check(lib.mdno_rollout(pack.ref, traj.data_ptr(), M, W, N, steps, aad.data_ptr(), 0, 8.0, cap, ws.data_ptr(), nb,
                                        eps.data_ptr(), status.data_ptr(), use_graph, stream.cuda_stream), "mdno_rollout")
            torch.cuda.synchronize()
            out[f"g{use_graph}"] = dict(traj=traj[W:], eps=eps, status=status)
        return out

    got = both_fills(run)
    assert same_bits(got["g0"]["traj"], got["g1"]["traj"]) and int(got["g1"]["status"]) == 0
    close(got["g1"]["traj"], _oracle_rollout(O, sd, wins, aa, steps), name="mdno_rollout")


# =============================================================================== scoring
@gpu
@pytest.mark.parametrize("S,M,N", [(3, 1, 1), (1, 3, 27), (5, 3, 65), (3, 5, 129)])
def test_scoring(dev, O, S, M, N):
    from test_gpu_forecast import frames_for, mse_bound, mse_ref, oracle_counts
    from molecular_dynamics_neural_operator_amd.forecast import contact_maps, score_forecast
    frames, truth = frames_for(N, S, M, seed=N + S)
    per_member = np.ascontiguousarray(np.broadcast_to(truth[:, None], frames.shape))

    def run(G):
        f, q, qm = G.place(torch.from_numpy(frames).to(dev)), G.place(torch.from_numpy(truth).to(dev)), G.place(torch.from_numpy(per_member).to(dev))
        out = {}
        for form in ("auto", "lds", "tiled"):
            for tag, tr in (("shared", q), ("own", qm)):
                sc = score_forecast(f, tr, 8.0, form=form)
                out[f"{form}.{tag}"] = dict(mse=sc.mse, rmsd=sc.rmsd, contacts=sc.contacts, first=sc.first_nonfinite)
        out["maps"] = contact_maps(f, 8.0)
        return out

    got = both_fills(run)
    want_counts = np.array([[oracle_counts(O, frames[s, m], truth[s], 8.0) for m in range(M)] for s in range(S)])
    want_mse = mse_ref(frames, truth)
    for key in [k for k in got if k != "maps"]:
        sc = got[key]
        assert np.array_equal(sc["contacts"].numpy(), want_counts), key
        rel = np.abs(sc["mse"].numpy() - want_mse) / np.where(want_mse > 0, want_mse, 1.0)
        assert rel.max() <= mse_bound(N), (key, rel.max())
        assert bool(torch.isfinite(sc["rmsd"]).all()) and sc["first"].tolist() == [-1] * M
        assert same_bits(sc["contacts"], got["auto.shared"]["contacts"])
    maps = got["maps"].numpy()
    for s in range(S):
        for m in range(M):
            ei = O.radius_graph_coo(frames[s, m], 8.0)
            want = np.zeros((N, N), dtype=np.uint8)
            want[ei[0], ei[1]] = 1
            assert maps[s, m].tobytes() == want.tobytes()


# =============================================================================== training
def _train_case(B, N, k, seed):
    from test_gpu_model_shapes import _train_samples
    return _train_samples(dict(atoms=N, batch=B, window=4, nemb=20, cutoff=8.0, out=3), seed)


@gpu
@pytest.mark.parametrize("mode", ["f32", "split_bf16", "split_f16", "bf16"])
@pytest.mark.parametrize("B,N", [(3, 33), (1, 1)])
def test_train_step(dev, O, B, N, mode):
    """train_forward + backward (node prologue and fc2 included) on a ragged batch: loss, output and every parameter
    gradient against the oracle's train step in fp64 (bf16: tests/bf16_replica.py), as tests/test_gpu_training.py.

    The bf16 replica rounds fp64 sums where the device rounds fp32 ones, so a stored value on a bf16 tie can fall to
    the other side inside the reference.  The bf16 case therefore first establishes, on the host, that the reference is
    well conditioned on its batch: the replica evaluated in fp32 agrees with the replica in fp64 to 0.3 of each bound
    (the share of a bound left to the reference's own rounding; the device gets the rest)."""
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN, LpLoss
    samples = _train_case(B, N, 128, 8101 + N)
    torch.manual_seed(3)
    model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
    with torch.no_grad():
        for p_ in model.conv1.net.layers[4].parameters():
            p_.mul_(0.2)
    model.to(dev).train()
    if mode == "bf16":
        model.train_precision = "bf16"
    else:
        model.gemm_mode = mode
    y = torch.cat([s.y for s in samples])

    def run(G):
        from molecular_dynamics_neural_operator_amd.dataset import PairData
        model.zero_grad(set_to_none=True)
        for p_ in model.parameters():          # parameters and every sample field between bands too
            p_.data = G.place(p_.data)
        placed = [PairData(**{f: G.place(getattr(s, f).to(dev)) for f in ("x_aminoacid", "x_position", "y", "edge_attr", "edge_index")})
                  for s in samples]
        out = model(placed)
        loss = LpLoss(size_average=False)(out.view(B, -1), G.place(y.to(dev)).view(B, -1))
        loss.backward()
        return dict(out=out, loss=loss, grads={n: p_.grad for n, p_ in model.named_parameters()})

    got = both_fills(run)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    as_dicts = [dict(x_position=s.x_position, x_aminoacid=s.x_aminoacid, y=s.y, edge_index=s.edge_index, edge_attr=s.edge_attr)
                for s in samples]
    if mode == "bf16":
        from bf16_replica import train_step_bf16
        want_loss, want_out, want_grads = train_step_bf16(O, sd, as_dicts, 2)
        tol_out, tol_g = 1e-4, 1e-3         # test_bf16_model_gradients_vs_fp64_replica's bounds against the replica
        _, out32, grads32 = train_step_bf16(O, sd, as_dicts, 2, dtype=torch.float32)
        own = rel_err(out32, want_out), max(rel_err(grads32[n], want_grads[n]) for n in want_grads)
        print(f"bf16 replica, fp32 against fp64: out {own[0]:.2e}, worst gradient {own[1]:.2e}")
        assert own[0] <= 0.3 * tol_out and own[1] <= 0.3 * tol_g, f"the reference is ill-conditioned on this batch: {own}"
    else:
        want_loss, want_out, want_grads = O.train_step(sd, as_dicts, 2)
        tol_out, tol_g = 1e-5, 1e-4
    assert abs(float(got["loss"]) - want_loss) < max(tol_out, 1e-5) * abs(want_loss)
    assert rel_err(got["out"], want_out) < tol_out
    for name, g_ in got["grads"].items():
        assert g_ is not None and rel_err(g_, want_grads[name]) < tol_g, (name, rel_err(g_, want_grads[name]))


@gpu
@pytest.mark.parametrize("B,D", [(1, 3), (37, 1512)])
def test_lploss(dev, O, B, D):
    from molecular_dynamics_neural_operator_amd.graph_kernel import LpLoss
    g = _gen(6, B, D)
    y = torch.randn(B, D, generator=g) * 5.0
    x = y + 0.3 * torch.randn(B, D, generator=g)

    def run(G):
        xd = G.place(x.to(dev)).requires_grad_(True)
        loss, mse = LpLoss(size_average=False).rel_with_mse(xd, G.place(y.to(dev)))
        (loss * 3.0).backward()
        return dict(loss=loss, mse=mse, grad=xd.grad)

    got = both_fills(run)
    x64 = x.double().requires_grad_(True)
    want = O.lp_loss_rel(x64, y.double(), size_average=False)
    (want * 3.0).backward()
    assert float(got["loss"]) == pytest.approx(float(want), rel=2e-6)
    assert float(got["mse"]) == pytest.approx(float(((x.double() - y.double()) ** 2).mean()), rel=2e-6)
    assert rel_err(got["grad"], x64.grad) < 2e-6


@gpu
def test_device_trajectory_batch(dev, tmp_path):
    from conftest import load_golden, write_golden_trajectory
    from molecular_dynamics_neural_operator_amd.dataset import ContactMapDataset
    from molecular_dynamics_neural_operator_amd.training import DeviceTrajectory, collate
    z = load_golden("rollout_20.npz")
    path = tmp_path / "traj.npz"
    write_golden_trajectory(path, z)
    dset = ContactMapDataset(str(path), window_size=4, horizon=3)
    idx = [len(dset) - 1, 0, 7, 7, 3]

    def run(G):
        b = DeviceTrajectory(dset, dev).batch(idx)
        return {f: getattr(b, f) for f in ("x_position", "y", "edge_index", "edge_attr", "x_aminoacid")}

    got = both_fills(run)
    want = collate([dset[i] for i in idx])
    for f, v in got.items():
        assert torch.equal(v, getattr(want, f)), f


@gpu
def test_adam(dev):
    """training.Adam over parameters of 1, 3, 4,097 and 1024 x 1025 elements, one of them without a gradient, two steps,
    against torch.optim.Adam in fp64 (tests/test_gpu_training.py: max error relative to the largest entry < 3e-6)."""
    from molecular_dynamics_neural_operator_amd.training import Adam as MdnoAdam
    gen = _gen(7)
    shapes = [(1,), (3,), (4097,), (1024, 1025)]
    init = [torch.randn(*sh, generator=gen) for sh in shapes]
    grads = [[torch.randn(*sh, generator=gen) for sh in shapes] for _ in range(2)]
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)

    def steps(params, opt, place):
        for s in range(2):
            for i, p_ in enumerate(params):
                p_.grad = None if (i == 1 and s == 1) else place(grads[s][i])
            opt.step()

    def run(G):
        params = [torch.nn.Parameter(G.place(t_.to(dev))) for t_ in init]
        steps(params, MdnoAdam(params, **kw), lambda t_: G.place(t_.to(dev)))
        return [p_.detach() for p_ in params]

    got = both_fills(run)
    exact = [torch.nn.Parameter(t_.double()) for t_ in init]
    steps(exact, torch.optim.Adam(exact, **kw), lambda t_: t_.double())
    for a_, c_ in zip(got, exact):
        ref = c_.detach()
        assert float((a_.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)) < 3e-6, tuple(a_.shape)


@gpu
def test_pack_unpack_abutting_slots(dev):
    """Slots that abut exactly, the last one ending at the end of the flat buffer; an int entry zero-fills its slot."""
    from molecular_dynamics_neural_operator_amd import ops
    gen = _gen(8)
    sizes = [1, 3, 4097, 64, 255]
    ts = [torch.randn(n, generator=gen) for n in sizes]
    offs = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)])[:-1]]
    total = sum(sizes)

    def run(G):
        src = [G.place(t_.to(dev)) for t_ in ts]
        flat = torch.empty(total, device=dev)
        ops.pack_tensors(src[:3] + [sizes[3]] + src[4:], flat, offs)
        back = [torch.empty(n, device=dev) for n in sizes]
        ops.unpack_tensors(flat, back, offs)
        return dict(flat=flat, back=back)

    got = both_fills(run)
    want = torch.cat(ts[:3] + [torch.zeros(64)] + ts[4:])
    assert torch.equal(got["flat"], want)
    for i, b in enumerate(got["back"]):
        assert torch.equal(b, want[offs[i]:offs[i] + sizes[i]])


# =============================================================================== undersized workspaces
def _undersize_calls(dev):
    """entry point -> a call that reaches it through the Python layer (inputs made outside the guard's bookkeeping)."""
    from molecular_dynamics_neural_operator_amd import ops
    from molecular_dynamics_neural_operator_amd.forecast import score_forecast
    from molecular_dynamics_neural_operator_amd.rollout import RolloutEngine
    from molecular_dynamics_neural_operator_amd.weights import near_identity_state_dict
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    bf = lambda t_: t_.to(torch.bfloat16)
    ei = torch.randint(0, 20, (2, 90), generator=g).to(dev)
    gr = ops.coo_to_csr(ei, 20)
    sd = near_identity_state_dict(64, 128, seed=1, kernel_gain=1e-2, feature_gain=0.1, kernel_to_coords=1.0)
    pack = ops.ParamPack(sd, 2, dev, gemm_mode="split_f16")
    frames, aa = rn(3, 1, 20, 3), torch.randint(0, 20, (20,), generator=g).to(dev)
    pos = frames[2].reshape(20, 3)
    w = [rn(128, 6), rn(128), rn(128, 128), rn(128), rn(4096, 128), rn(4096)]

    def rollout_plan():
        from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
        model = KernelNN(64, 128, 2, 6, 7, 3, 20, 4)
        model.load_state_dict(sd)
        model.eval().to(dev)
        model.conv_mode = "materialized"             # (no probe graph: nothing but the plan is built before the refusal)
        # (an all-zero window: the engine's zero-initialised trajectory buffer must still be all zero after the refusal)
        RolloutEngine(model, 1, 20, 3, 8.0, max_steps=2, edge_cap=400, device=dev).run(torch.zeros_like(frames), aa, 2)

    def rollout_c():
        from molecular_dynamics_neural_operator_amd import _lib
        lib = _lib.load()
        traj = torch.empty((5, 1, 20, 3), device=dev)
        nb = lib.mdno_rollout_workspace_bytes(pack.ref, 1, 20, 400)
        ws, eps, st = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.mdno_rollout(pack.ref, traj.data_ptr(), 1, 3, 20, 2, aa.data_ptr(), 0, 8.0, 400, ws.data_ptr(), nb,
                                    eps.data_ptr(), st.data_ptr(), 0, _lib.stream_ptr(dev)), "mdno_rollout")

    x0 = ops.node_prologue(pack, frames, aa)
    rg = ops.radius_graph(pos, 20, 8.0)
    return {
        "mdno_coo_to_csr": lambda: ops.coo_to_csr(ei, 20),
        "mdno_csr_by_source": lambda: ops.source_sorted(gr, 20),
        "mdno_edge_mlp_fwd": lambda: ops.edge_mlp(w, 6, 128, 4096, gr, edge_pos=pos, gemm_mode="split_f16"),
        "mdno_kernelnn_fwd": lambda: ops.kernelnn_forward(pack, frames, aa, rg, edge_pos=pos),
        "mdno_rollout": rollout_c,
        "mdno_rollout_plan_create": rollout_plan,
        "mdno_linear_split_fwd": lambda: ops.linear(rn(70, 64), rn(128, 64), None, gemm_mode="split_bf16"),
        "mdno_linear_split_f16_fwd": lambda: ops.linear(rn(70, 64), rn(128, 64), None, gemm_mode="split_f16"),
        "mdno_gemm_atb": lambda: ops.gemm_atb(rn(70, 64), rn(70, 6)),
        "mdno_gemm_atb_split_f16": lambda: ops.gemm_atb(rn(70, 256), rn(70, 256), gemm_mode="split_f16"),
        "mdno_colsum": lambda: ops.colsum(rn(70, 64)),
        "mdno_nnconv_bwd_root_pair": lambda: ops.nnconv_bwd_root_pair(rn(4, 20, 64), rn(4, 20, 64)),
        "mdno_nnconv_bwd_root": lambda: ops.nnconv_bwd_root(rn(70, 64), rn(70, 64)),
        "mdno_linear_bf16_fwd": lambda: ops.linear_bf16(bf(rn(70, 64)), rn(128, 64), None),
        "mdno_linear_bf16_masked": lambda: ops.linear_bf16_relu_bwd(bf(rn(70, 64)), rn(256, 64), bf(rn(70, 256))),
        "mdno_gemm_atb_bf16": lambda: ops.gemm_atb_bf16(bf(rn(70, 128)), bf(rn(70, 128))),
        "mdno_nnconv_bwd_we_colsum": lambda: ops.nnconv_bwd_we(rn(2, 20, 64), rn(2, 20, 64), gr, with_colsum=True),
        "mdno_nnconv_bwd_we_bf16_colsum": lambda: ops.nnconv_bwd_we_bf16(rn(2, 20, 64), rn(2, 20, 64), gr, with_colsum=True),
        "mdno_colsum_bf16": lambda: ops.colsum_bf16(bf(rn(70, 128))),
        "mdno_colsum_atb_bf16": lambda: ops.colsum_atb_bf16(bf(rn(70, 128)), rn(70, 6)),
        "mdno_node_prologue_bwd": lambda: ops.node_prologue_bwd(pack, frames, aa, x0, rn(20, 64)),
        "mdno_fc_out_bwd": lambda: ops.fc_out_bwd(rn(20, 64), rn(3, 64), rn(20, 3)),
        "mdno_forecast_score": lambda: score_forecast(rn(3, 2, 20, 3), rn(3, 20, 3), 8.0),
    }


@pytest.fixture(scope="module")
def undersize_calls(dev):
    return _undersize_calls(dev)


@gpu
@pytest.mark.parametrize("entry", sorted(set(WORKSPACE_OF) - {"mdno_radius_graph_csr_ws"}))
def test_undersized_workspace_is_refused(dev, undersize_calls, entry):
    """One byte less than the entry's *_workspace_bytes function states: MDNO_EWORKSPACE before any device work — every
    output allocated for the call still holds the fill, and the guards are intact.  (mdno_radius_graph_csr_ws documents
    a fallback instead: test_radius_graph_cell_list.)"""
    from molecular_dynamics_neural_operator_amd import _lib
    call = undersize_calls[entry]
    torch.cuda.synchronize()
    for fill in FILLS:
        with Guard(fill, undersize={entry: WORKSPACE_OF[entry]}) as G:
            with pytest.raises(_lib.MdnoError, match=r"\(code -3\)"):
                call()
            assert G.undersized and G.undersized[-1][0] == entry and "mdno_last_error" in G.calls, G.calls[-4:]
            G.verify()
            G.untouched()


# =============================================================================== completeness, on the device
@gpu
def test_recorded_entry_points_equal_the_table():
    """Runs last: what the guards of this file saw is what COVERAGE says (skipped when a selection left cases out)."""
    gpu_tests = {k for k, v in globals().items() if k.startswith("test_") and callable(v)
                 and any(m.name == "gpu" for m in getattr(v, "pytestmark", []))} - {"test_recorded_entry_points_equal_the_table"}
    if not gpu_tests <= RAN:
        pytest.skip(f"not every case of this file ran in this process: {sorted(gpu_tests - RAN)}")
    decls = guarded.header_functions()
    writers = {n for n in RECORDED if guarded.writes_memory(decls[n])}
    assert writers - set(EXEMPT) == set(COVERAGE), (sorted(set(COVERAGE) - writers), sorted(writers - set(EXEMPT) - set(COVERAGE)))
