"""include/mdno_train.h — the second public header of libmdno.so (training on dense graphs): what is particular to it
(that header, table and exports agree is tests/test_cabi_tables.py's), and `train_conv_mode="factored"` is refused on
a CPU model, before any device work, where the factored training path does not apply.  No GPU needed."""
import pytest
import torch

from cabi import INCLUDE, lib  # noqa: F401  (lib: the fixture)

HEADER = INCLUDE / "mdno_train.h"


def test_train_header_table_and_exports_agree(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    assert len(_lib.TRAIN_SIGNATURES) == 6 and all(n.startswith("mdno_train_") for n in _lib.TRAIN_SIGNATURES)
    assert lib.mdno_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1
    assert "#define MDNO_TRAIN_ABI_VERSION 1" in HEADER.read_text()


def test_train_entry_points_validate_before_device_work(lib):
    from molecular_dynamics_neural_operator_amd import _lib
    assert lib.mdno_train_moment_h_floats(300, 128) == 384 * 128 and lib.mdno_train_moment_h_floats(0, 128) == 128 * 128
    assert lib.mdno_train_moment_fwd_workspace_bytes(100, 100, 1000, 0) == 0          # untileable k
    assert lib.mdno_train_moment_bwd_workspace_bytes(100, 100, 1000) == 0
    small, big = (lib.mdno_train_moment_bwd_workspace_bytes(100, 128, e) for e in (1000, 2000))
    assert 0 < small < big and (big - small) <= 1000 * (128 * 4 + 256) + 128 * 128 * 4 + 1024      # 4 k + 256 B per edge
    rc = lib.mdno_train_moment_fwd(*([None] * 3), 1, 6, 128, 0, *([None] * 9), 1, *([None] * 4), 1, *([None] * 3), 0, None)
    assert rc == _lib.EINVAL and b"null pointer" in lib.mdno_last_error()
    rc = lib.mdno_train_moment_bwd(*([None] * 7), 1, 1, 128, 1, 0, *([None] * 10), 0, None)
    assert rc == _lib.EINVAL and b"null pointer" in lib.mdno_last_error()


@pytest.mark.parametrize("case", ["bf16", "ker_width_100", "width_32"])
def test_factored_refusals_on_cpu_model(case):
    from molecular_dynamics_neural_operator_amd.graph_kernel import KernelNN
    from molecular_dynamics_neural_operator_amd.training import check_trainable, train_forward
    from molecular_dynamics_neural_operator_amd.dataset import PairData
    width, k = (32, 128) if case == "width_32" else (64, 100 if case == "ker_width_100" else 128)
    torch.manual_seed(0)
    model = KernelNN(width, k, 1, 6, 7, 3, 20, 4)
    model.train_conv_mode = "factored"
    if case == "bf16":
        model.train_precision = "bf16"
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with pytest.raises(NotImplementedError) as err:
        check_trainable(model, 10)
    if case == "bf16":
        assert "out of scope" in str(err.value)
    n = 5
    ei = torch.stack([torch.arange(n), torch.arange(n)])
    sample = PairData(torch.zeros(n, dtype=torch.long), torch.zeros(10, n, 3), torch.zeros(n, 3), torch.zeros(n, 6), ei)
    with pytest.raises(NotImplementedError):
        train_forward(model, [sample])
    assert getattr(model, "_train_status", None) is None
    for name, p in model.named_parameters():
        assert p.grad is None and torch.equal(p, before[name]) and p.device.type == "cpu", name
    # the default and "auto" are not refused by the new checks
    model.train_conv_mode = "auto"
    if case != "width_32":
        check_trainable(model, 10)
    model.train_conv_mode = "bogus"
    if case != "width_32":
        from molecular_dynamics_neural_operator_amd._lib import MdnoError
        with pytest.raises(MdnoError):
            check_trainable(model, 10)
