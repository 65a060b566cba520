"""Writes tests/golden/ntxent_golden.npz: the reference's NTXentLoss (simclr/loss/nt_xent.py, imported UNMODIFIED from a
checkout of binli123/dsmil-wsi) evaluated in fp64 with autograd on the seeded inputs of tests/ntxent_cases.GOLDEN_CASES.

    python tests/golden/make_ntxent_golden.py /path/to/dsmil-wsi

Per case: <name>/zis, <name>/zjs (fp32 inputs), <name>/loss, <name>/g_zis, <name>/g_zjs (fp64).  Data only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ntxent_cases as nc  # noqa: E402


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_nt_xent", os.path.join(ref_root, "simclr", "loss", "nt_xent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for case in nc.GOLDEN_CASES:
        zis, zjs = nc.make_inputs(case)
        a = torch.tensor(zis, dtype=torch.float64, requires_grad=True)
        b = torch.tensor(zjs, dtype=torch.float64, requires_grad=True)
        crit = mod.NTXentLoss(torch.device("cpu"), case[0], case[2], bool(case[3]))
        loss = crit(a, b)
        loss.backward()
        name = nc.case_name(case)
        out[name + "/zis"], out[name + "/zjs"] = zis, zjs
        out[name + "/loss"] = np.float64(loss.item())
        out[name + "/g_zis"], out[name + "/g_zjs"] = a.grad.numpy(), b.grad.numpy()
        print(name, loss.item())
    path = os.path.join(HERE, "ntxent_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
