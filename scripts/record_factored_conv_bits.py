#!/usr/bin/env python
"""Record tests/golden/factored_conv_bits.npz: the raw uint32 images of the factored conv's output for the cases of
tests/test_gpu_conv_chain_partials.py (which builds the inputs and runs the forward: this script only loops and saves).

Run it on the GPU on the commit whose bits are to be kept — it was run once, on the commit before project_f16_kernel
began to add a chain's slices itself:
    python scripts/record_factored_conv_bits.py [OUT.npz]
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "tests")]


def main():
    spec = importlib.util.spec_from_file_location("chain_cases", REPO / "tests" / "test_gpu_conv_chain_partials.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else mod.GOLDEN_FILE
    dev = torch.device("cuda:0")
    bits = {}
    for case in mod.CASES:
        name = mod.case_id(case)
        bits[name] = mod.run_case(case, dev)
        again = mod.run_case(case, dev)
        assert np.array_equal(bits[name], again), f"{name}: two runs of the same forward differ"
        print(f"{name}: {bits[name].shape[0]} rows, {int((bits[name] == 0).sum())} zero words")
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **bits)
    print(f"wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
