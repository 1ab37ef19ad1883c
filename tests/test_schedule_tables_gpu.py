"""The static schedule of every handle kind, entry by entry, against a recorded table (tests/schedule_tables.json, and
tests/schedule_tables_xform.json for the handles of XFORM_CASES).

csrc/net.cpp builds, per handle, a list of kernels with their accounting rows, a liveness-planned arena, a packed weight blob and a
list of debug taps.  All of it is decided on the host when the handle is created, and all of it can be read back without running a
forward: the number of entries, every entry's (kind, bytes, flops) row and description, the device bytes (weights + arena, so every
allocation and every blob entry counts), the model bytes and flops, and the taps.  A change to the builder that is meant to leave the
schedule alone -- moving code between functions, sharing a stem or a head between kinds -- must leave every one of these figures as it
was; an entry that moved, an allocation that grew or a tap that went missing shows here by name and position.

CASES reaches every branch of the builder with tiny handles (and a two-channel encoder, whose in_conv row has always shown one input
channel): base 32 (24 for the padded widths), 2 clips, the shortest length each
topology takes (256 for the default nine levels, 512 for the default classifier, the lengths of tests/enroll_ref.py and
tests/backward_ref.py for the custom ones, 800 for the MFCC front end), in fp32 and, where the kind has a 2-byte mode, fp16.
None of them is wide enough for the hoisted prologue (`xform` entries): XFORM_CASES reaches it, in a table of its own so that the first
one stays as it was recorded, byte for byte.

The tables are written by `python tests/test_schedule_tables_gpu.py --record` (handles are created on the device, so on a GPU machine)
and never by the test.  Equal rows are stored once per file (`rows`) and referred to by index, which keeps the files small."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "schedule_tables.json")
XFORM_TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "schedule_tables_xform.json")
B = 2
SMALL = dict(channel_mult=(1, 2, 2), depth_mult=1, middle_dilations=(4,))
BOTH, F32 = ("fp32", "fp16"), ("fp32",)


def _models():
    from vq_voice_swap_amd import Classifier, EncoderPredictor
    from vq_voice_swap_amd.conv_encoder import ConvMFCCEncoder
    from vq_voice_swap_amd.unet import ResBlockModule, UNetEncoder, UNetPredictor

    return dict(rb=ResBlockModule, pred=UNetPredictor, enc=UNetEncoder, clf=Classifier, ep=EncoderPredictor, mfcc=ConvMFCCEncoder)


# (id, constructor key, args, kwargs, T, precisions, extras): cond_code = UNetPredictor._cond_code (0: T / 256 rows, 1: T / 320 rows,
# 1000 + n: n rows); grad = the predictor-gradient handle of UNetPredictor._grad_handle in place of the forward handle
CASES = [
    ("rb_plain", "rb", (32,), {}, 256, BOTH, {}),
    ("rb_emb", "rb", (32, 128), {}, 256, BOTH, {}),
    ("rb_emb_widen", "rb", (32, 128, 64), {}, 256, BOTH, {}),
    ("pred_plain", "pred", (32,), {}, 256, BOTH, {}),
    ("pred_labels", "pred", (32,), dict(num_labels=4), 256, BOTH, {}),
    ("pred_cond_t256", "pred", (32,), dict(cond_channels=32), 256, BOTH, dict(cond_code=0)),
    ("pred_cond_t320", "pred", (32,), dict(cond_channels=32), 256, BOTH, dict(cond_code=1)),
    ("pred_cond_abs5", "pred", (32,), dict(cond_channels=32), 256, BOTH, dict(cond_code=1005)),
    ("pred_out32", "pred", (32,), dict(out_channels=32), 256, BOTH, {}),
    ("pred_custom", "pred", (32,), dict(num_labels=4, **SMALL), 592, BOTH, {}),
    ("pred_padded24", "pred", (24,), dict(num_labels=4), 256, BOTH, {}),
    ("enc_default", "enc", (32,), dict(out_channels=64), 256, BOTH, {}),
    ("enc_padded24", "enc", (24,), dict(out_channels=64), 256, BOTH, {}),
    ("enc_custom", "enc", (32,), dict(channel_mult=(1, 2, 4), out_dilations=(2, 8), depth_mult=1, out_channels=64), 592, BOTH, {}),
    ("enc_stereo", "enc", (32,), dict(channel_mult=(1, 2), depth_mult=1, in_channels=2, out_channels=64), 256, BOTH, {}),
    ("clf_default", "clf", (5,), dict(base_channels=32), 512, BOTH, {}),
    ("clf_custom", "clf", (5,), dict(base_channels=32, channel_mult=(1, 2, 2, 4), output_mult=8, depth_mult=1), 592, BOTH, {}),
    ("encpred", "ep", (32, 256), dict(num_latents=40, bottleneck_dim=32), 256, BOTH, {}),
    ("mfcc_v1", "mfcc", (32,), dict(version=1), 800, F32, {}),
    ("mfcc_v2", "mfcc", (32,), dict(version=2), 800, F32, {}),
    ("grad_plain", "pred", (32,), dict(num_labels=4, **SMALL), 592, F32, dict(grad=True)),
    ("grad_cond", "pred", (32,), dict(num_labels=4, cond_channels=32), 256, F32, dict(grad=True, cond_code=0)),
]
# The hoisted prologue (`xform` entries).  pred_wide: widths of 512 from level 1 -- fp32 hoists both convolutions of every block from
# 512 output channels up (the x0.5 block at 512: an `avg` entry), fp16 only conv 1 of the up blocks whose concatenated input is 1024
# wide (no `avg`: a resizing block never concatenates).  rb_avg1024: the one place fp16 hoists WITH the average pool, a x0.5 block more
# than 640 channels wide.
XFORM_CASES = [
    ("pred_wide", "pred", (32,), dict(channel_mult=(1, 16, 16), depth_mult=1, middle_dilations=(4,)), 256, BOTH, {}),
    ("rb_avg1024", "rb", (1024,), dict(scale_factor=0.5), 256, BOTH, {}),
]
FILES = ((TABLES, CASES), (XFORM_TABLES, XFORM_CASES))


def ids(cases):
    return [f"{c[0]}.{p}" for c in cases for p in c[5]]


CASE_IDS = ids(CASES) + ids(XFORM_CASES)


def make_module(case, prec):
    """The module of a case on the CPU with name-seeded weights, in precision mode `prec`."""
    from vq_voice_swap_amd.det_init import det_init_

    cid, key, args, kw, _T, _precs, extra = case
    m = _models()[key](*args, **kw)
    det_init_((f"sched.{cid}.{k}", v) for k, v in m.named_parameters())  # (buffers -- the MFCC front end's tables -- stay as built)
    m.eval()
    m.set_precision(prec)
    if "cond_code" in extra:  # (no public setter: forward() derives the code from the length of `cond`, and _NativeModule.handle() /
        m._cond_code = extra["cond_code"]  # UNetPredictor._cfg() read it into the handle key and vqvs_cfg.reserved[3])
    return m


def make_handle(case, m, dev):
    T = case[4]
    return m._grad_handle(dev, B, T) if case[6].get("grad") else m.handle(dev, B, T)


def tables(h, T):
    """Everything the schedule builder decided for handle `h`, as JSON types."""
    info, desc = h.op_info(B, T), h.op_desc()
    assert len(info) == len(desc) == h.kernel_count()
    return dict(kernel_count=h.kernel_count(), ops=[[k, by, fl, d] for (k, by, fl), d in zip(info, desc)], device_bytes=h.device_bytes(),
                model_bytes=h.model_bytes(B, T), flops=h.flops(B, T), taps=[list(t) for t in h.taps()])


def live(cid):
    name, prec = cid.rsplit(".", 1)
    case = next(c for c in CASES + XFORM_CASES if c[0] == name)
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m = make_module(case, prec)
    got = tables(make_handle(case, m, torch.device("cuda:0")), case[4])
    m.invalidate()
    return got


@pytest.fixture(scope="module")
def recorded():
    want = {}
    for path, cases in FILES:
        with open(path) as f:
            z = json.load(f)
        assert sorted(z["cases"]) == sorted(ids(cases)), f"{os.path.basename(path)} does not hold the case list of this file"
        for cid, t in z["cases"].items():
            want[cid] = dict(t, ops=[z["rows"][i] for i in t["ops"]])
    return want


@pytest.mark.parametrize("cid", CASE_IDS)
def test_schedule_tables(cid, recorded):
    want = recorded[cid]
    got = live(cid)
    assert got["kernel_count"] == want["kernel_count"]
    for i, (g, w) in enumerate(zip(got["ops"], want["ops"])):
        assert g == w, f"{cid}: schedule entry {i} is {g}, recorded {w}"
    assert got["taps"] == want["taps"]
    for k in ("device_bytes", "model_bytes", "flops"):
        assert got[k] == want[k], (cid, k, got[k], want[k])
    assert got == want


def record(path, case_ids):
    rows, index, cases = [], {}, {}
    for cid in case_ids:
        t = live(cid)
        ops = []
        for r in t["ops"]:
            key = json.dumps(r)
            if key not in index:
                index[key] = len(rows)
                rows.append(r)
            ops.append(index[key])
        t["ops"] = ops
        cases[cid] = t
        print(f"{cid}: {t['kernel_count']} entries, {t['device_bytes']} device bytes, {len(t['taps'])} taps", flush=True)
    with open(path, "w") as f:
        json.dump(dict(rows=rows, cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {len(cases)} handles, {len(rows)} distinct rows")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_schedule_tables_gpu.py --record")
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    for path, cases in FILES:
        record(path, ids(cases))
