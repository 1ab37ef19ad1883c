"""One block run of tests/test_groupnorm_gpu.py in an interpreter of its own: the library reads VQVS_WS_GN once per process, so the two
builders of a (scale, shift) table -- gn_prepare_kernel and the consuming convolution's gn_table -- are compared across processes.

    python groupnorm_child.py '<json spec>' <out.pt>

spec["what"] == "table": the fp16 block of spec["case"] (groupnorm_ref.BLOCK_CASES) on N(0, 1); saves the output, every GroupNorm's
partials and fused flag.  spec["what"] == "guard": ResBlockModule(64, 128, None, 1.0, 1), fp16, L = 256, an input of constant magnitude
spec["magnitude"] with a zero-mean sign pattern; saves the status word and the fused flags.  Prints GN_CHILD_OK when it is done."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import groupnorm_ref as gr  # noqa: E402
from vq_voice_swap_amd.det_init import det_init_  # noqa: E402
from vq_voice_swap_amd.unet import ResBlockModule  # noqa: E402


def main():
    spec, out_path = json.loads(sys.argv[1]), sys.argv[2]
    dev = torch.device("cuda:0")
    if spec["what"] == "table":
        cin, cout, scale, dil, L, B, _modes = gr.BLOCK_CASES[spec["case"]]
        m = ResBlockModule(cin, gr.EMB, cout, scale, dil)
        det_init_((f"gn.{spec['case']}." + k, v) for k, v in m.block.state_dict().items())
        x, e = gr.block_input(spec["case"], "n01")
    else:
        B, L = 3, 256
        m = ResBlockModule(64, gr.EMB, None, 1.0, 1)
        det_init_(("gn.guard." + k, v) for k, v in m.block.state_dict().items())
        sign = 1.0 - 2.0 * ((torch.arange(L)[None, :] + torch.arange(64)[:, None]) % 2).float()  # [64, L]: every channel sums to zero
        x = (float(spec["magnitude"]) * sign)[None].expand(B, 64, L).contiguous()
        e = torch.zeros(B, gr.EMB)
    m.set_precision("fp16")
    m.debug_taps = True
    h = m.handle(dev, B, L)
    h.status()  # (read and cleared)
    y = m(x.to(dev), e.to(dev)).cpu()
    status = h.status()
    infos = [h.gn_info(i, B, L) for i in range(h.gn_count())]
    res = dict(out=y, status=status, fused=[g["fused"] for g in infos], infos=infos,
               partials=[[h.gn_partials(i, B, L, s) for s in range(len(g["srcs"]))] for i, g in enumerate(infos)],
               tables=[h.gn_table(i, B, L) for i in range(len(infos))], film=h.read_film(B))
    torch.save(res, out_path)
    print("GN_CHILD_OK", flush=True)


if __name__ == "__main__":
    main()
