"""Generate tests/golden/vae_model.npz from the reference's own test data (a companion of make_golden.py, which it leaves
untouched).  Run in the build container only (it reads the reference's tests/data, which never travels):

    python tests/golden/make_golden_vae.py

Stored is *data* only: the parameters and buffers of the TorchScript file inside input/models/vae_model.zip (keys
``param.<name>`` / ``buffer.<name>``) and its ``forward`` output on features_164x54.npz (``output``), evaluated here with
torch.jit.load.  No TorchScript file is committed: its archive holds the reference's code.
"""
import io
import os
import zipfile

import numpy as np
import torch

REF = "/root/reference"
DATA = os.path.join(REF, "deep_cartograph", "tests", "data")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    X = np.load(os.path.join(OUT, "features_164x54.npz"))["X"]
    out = {}
    with zipfile.ZipFile(os.path.join(DATA, "input", "models", "vae_model.zip")) as z:
        m = torch.jit.load(io.BytesIO(z.read("model/cv_weights.pt")))
    m.eval()
    for n, p in m.named_parameters():
        out[f"param.{n}"] = p.detach().numpy()
    for n, b in m.named_buffers():
        out[f"buffer.{n}"] = b.detach().numpy()
    with torch.no_grad():
        out["output"] = m(torch.from_numpy(X)).numpy()
    np.savez_compressed(os.path.join(OUT, "vae_model.npz"), **out)


if __name__ == "__main__":
    main()
