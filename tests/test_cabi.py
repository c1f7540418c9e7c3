"""The C-ABI library loads (no GPU needed): the version number, the parameter struct's layout, argument validation before
any device work, the tie between the library and the tree it was built from, and the host logic of the conv mode.  That
include/mdno.h, its ctypes table and the exports agree is tests/test_cabi_tables.py's, for every header alike.  No compute
calls here."""
import ctypes

import pytest

from cabi import CSRC, declared_functions, INCLUDE, lib  # noqa: F401  (lib: the fixture)


def test_mdno_h_declares_at_least_the_first_rounds_entry_points():
    assert len(declared_functions(INCLUDE / "mdno.h")) >= 17


def test_abi_version_struct_layout_and_error_string(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    assert lib.mdno_abi_version() == _lib.ABI_VERSION == 15
    # 12 int32 + 27 pointers, no padding surprises
    assert ctypes.sizeof(_lib.KernelNNParams) == 12 * 4 + 27 * 8
    # argument validation happens before any device work: exercise it without a GPU
    rc = lib.mdno_nnconv_fwd(None, None, None, 1, None, None, None, 64, 64, 1, 0, None, None)
    assert rc == _lib.EINVAL and b"null pointer" in lib.mdno_last_error()
    assert lib.mdno_edge_mlp_workspace_bytes(1024, 4096, 1000, _lib.GEMM_MODES["f32"]) == 2 * 1024 * 1024 * 4 + 512
    # split mode: 2 x 3 bf16 activation planes + the split weights; untileable shapes fall back to fp32 sizing
    # (+ the two fp16 planes of W1 and of W2, a 256-B line of range flags and one fp32 unscale factor per
    # weight row, used by SPLIT_F16; a launch of <= 1,024 rows also keeps fp16 images of h1 and h2 beside the
    # bf16 ones: its GEMMs choose between them themselves)
    assert lib.mdno_edge_mlp_workspace_bytes(1024, 4096, 1000, 0) == (2 * 3 * 1024 * 1024 * 2 + 3 * 2 * (1024 + 4096) * 1024
                                                                      + 2 * 2 * (1024 + 4096) * 1024 + 256
                                                                      + 4 * (1024 + 4096) + 2 * 2 * 1024 * 1024 * 2)
    assert lib.mdno_edge_mlp_workspace_bytes(1024, 4096, 2000, 0) == (2 * 3 * 2048 * 1024 * 2 + 3 * 2 * (1024 + 4096) * 1024
                                                                      + 2 * 2 * (1024 + 4096) * 1024 + 256
                                                                      + 4 * (1024 + 4096))
    assert lib.mdno_edge_mlp_workspace_bytes(1024, 4096, 1000, _lib.GEMM_MODES["split_f16"]) == \
        lib.mdno_edge_mlp_workspace_bytes(1024, 4096, 1000, 0)
    assert lib.mdno_edge_mlp_workspace_bytes(16, 64, 1000, 0) == 2 * 1024 * 16 * 4 + 512
    assert lib.mdno_kernelnn_workspace_bytes(None, 1, 1, 1) == 0
    with pytest.raises(_lib.MdnoError):
        _lib.check(rc, "nnconv")


def test_library_is_built_from_this_tree(lib, tmp_path, monkeypatch):
    """mdno_build_id() == the content hash of csrc/* + include/*.h as they are now (the .so is untracked but
    shipped to the GPU box: this is what ties it to HEAD); a library from other sources is refused at load."""
    from molecular_dynamics_neural_operator_amd import _lib
    want = _lib.source_build_id()
    assert want is not None and len(want) == 16
    assert lib.mdno_build_id().decode() == want
    stamp = (CSRC / "build" / "BUILD_ID").read_text().split()[0]
    assert stamp == want
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "source_build_id", lambda: "0" * 16)
    with pytest.raises(_lib.MdnoError, match="built from other sources"):
        _lib.load()


def test_conv_mode_resolution_is_host_logic(lib):
    """mdno_resolve_conv_mode (include/mdno.h MDNO_CONV_AUTO): factored where it applies (width 64,
    ker_width a multiple of 64) and, for auto, only from an edge capacity of 24,576 PER MEMBER on — a
    member takes the same path alone and inside any batch."""
    from molecular_dynamics_neural_operator_amd import _lib
    M, F, A = (_lib.CONV_MODES[k] for k in ("materialized", "factored", "auto"))

    def resolve(width, ker_width, mode, cap, members=1):
        p = _lib.KernelNNParams()
        p.width, p.ker_width, p.depth, p.ker_in, p.out_width, p.conv_mode = width, ker_width, 6, 6, 3, mode
        return lib.mdno_resolve_conv_mode(ctypes.byref(p), members, cap)

    assert resolve(64, 1024, A, 24575) == M and resolve(64, 1024, A, 24576) == F
    assert resolve(64, 1024, F, 100) == F and resolve(64, 1024, M, 10**6) == M
    assert resolve(32, 1024, A, 10**6) == M and resolve(32, 1024, F, 10**6) == M      # width != 64: never
    assert resolve(64, 1000, A, 10**6) == M                                            # untileable k
    assert resolve(64, 1024, A, 8 * 24576 - 8, members=8) == M and resolve(64, 1024, A, 8 * 24576, members=8) == F
    assert resolve(64, 1024, A, 64 * 784, members=64) == M                            # 64 x N=28: materialized
    assert lib.mdno_resolve_conv_mode(None, 1, 10**6) == M
