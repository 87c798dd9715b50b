"""Generate tests/golden/ref_imgloss.npz by EXECUTING the reference's image losses on the CPU:

  * utils/loss_utils.py  l1_loss, l2_loss, ssim (size_average True and False)
  * utils/image_utils.py psnr

on the (2,3,37,45) case of tests/imgloss_cases.py (inputs written by that module, float32).  Recorded: the two input images
and the five outputs, and the eleven taps of the reference's gaussian(11, 1.5).

Run in the build container only (needs /root/reference, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imgloss.py

Data only: inputs written by this repository's test module, outputs produced by the reference's code.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.dirname(HERE))
    import imgloss_cases as IC
    sys.path.insert(0, REF)
    from utils import image_utils as RI
    from utils import loss_utils as RL

    case = next(c for c in IC.cases() if c.shape == IC.GOLDEN_SHAPE and c.kind == "noise")
    x_np, y_np = IC.inputs(case)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    out = dict(img=x_np, ref=y_np, shape=np.array(IC.GOLDEN_SHAPE),
               l1=RL.l1_loss(x, y).numpy(), l2=RL.l2_loss(x, y).numpy(),
               ssim_mean=RL.ssim(x, y).numpy(), ssim_per_image=RL.ssim(x, y, size_average=False).numpy(),
               psnr=RI.psnr(x, y).numpy(), taps=RL.gaussian(11, 1.5).numpy())
    path = os.path.join(HERE, "ref_imgloss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
