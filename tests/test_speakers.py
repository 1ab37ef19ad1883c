"""Speaker vectors as inputs, the parts that need no device: the spec grammar, the tables the mix is called
with (blends, vector files, the null-label offset, the morph rule), the pseudo-voice rule against committed literals, voice files, the
scripts' flags, `convert_dataset.py --anonymize` with the model stubbed, the declarations and exports of the two entry points, their
refusals, and the numpy restatement of the mix against float64."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import speakers_ref as SR
from vq_voice_swap_amd import UNetPredictor, _native
from vq_voice_swap_amd import speakers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_num_threads(8)


# ---------------------------------------------------------------- the grammar
def test_parse_voice():
    assert S.parse_voice("7") == [(7, 1.0)]
    assert S.parse_voice("3:0.7,251:0.3") == [(3, 0.7), (251, 0.3)]  # as given: not renormalised
    assert S.parse_voice(" 3:2 , 4:-0.5 ") == [(3, 2.0), (4, -0.5)]
    assert S.parse_voice("@voice.npy") == [("voice.npy", 1.0)]
    assert S.parse_voice("@a.npy:0.5,7:0.5") == [("a.npy", 0.5), (7, 0.5)]
    assert S.parse_voice("@dir/b.c.npy:1e-1") == [("dir/b.c.npy", 0.1)]
    assert len(S.parse_voice(",".join(str(i) for i in range(8)))) == 8
    for bad in ("", " ", "a", "3:", "3:x", ",", "3,,4", "-1", "1.5", "@", "@:0.5", "3:nan", "3:inf", "3:0.5:1", "@a.npy:x",
                ",".join(str(i) for i in range(9))):
        with pytest.raises(ValueError) as e:
            S.parse_voice(bad)
        assert repr(bad) in str(e.value), (bad, str(e.value))  # the error names the text
    with pytest.raises(ValueError):
        S.parse_voice(None)
    assert S.single_label("7") == 7 and S.single_label(7) == 7
    assert S.single_label("7:0.5") is None and S.single_label("7,8") is None and S.single_label("@v.npy") is None
    entries = [(3, float(np.float32(0.7))), ("v.npy", float(np.float32(0.3)))]
    assert S.parse_voice(S.format_voice(entries)) == entries  # text that reads back to the same float32 weights


def test_mix_tables():
    idx, w, files = S.mix_tables([[(3, 0.7), (1, 0.3)], [(2, 1.0)], [("a.npy", 0.5), (0, 0.25), ("b.npy", 1.0)], [("a.npy", 2.0)]], 4)
    assert idx.dtype == np.int32 and w.dtype == np.float32 and files == ["a.npy", "b.npy"]
    assert idx.tolist() == [[3, 1, -1], [2, -1, -1], [4, 0, 5], [4, -1, -1]]
    assert w.tolist() == [[np.float32(0.7), np.float32(0.3), 0.0], [1.0, 0.0, 0.0], [0.5, 0.25, 1.0], [2.0, 0.0, 0.0]]
    idx, _, _ = S.mix_tables([[(2, 1.0)], [("a.npy", 1.0)]], 4, label_offset=1)  # the null label in front: speakers one row up
    assert idx.tolist() == [[3], [4]]
    for entries, offset in ([(4, 1.0)], 0), ([(3, 1.0)], 1):
        with pytest.raises(IndexError):
            S.mix_tables([entries], 4, offset)
    with pytest.raises(ValueError):
        S.mix_tables([[(0, 1.0)] * 17], 4)
    with pytest.raises(ValueError):
        S.mix_tables([], 4)


# ---------------------------------------------------------------- the morph rule
W, H, SR_HZ = 2048, 1536, 16000


def test_morph_entries():
    c = [(b * H + W / 2) / SR_HZ for b in range(3)]  # window centres: 0.064, 0.16, 0.256 s
    # n = 1: the one window's centre between the points
    (e,) = S.morph_entries([(0.0, "1"), (0.128, "2")], 1, W, H, SR_HZ)
    assert e == [(1, 0.5), (2, 0.5)]
    # a point before the first centre and one after the last: every window strictly between them
    got = S.morph_entries([(0.0, "1:0.5,0:0.5"), (1.0, "2")], 3, W, H, SR_HZ)
    for b, e in enumerate(got):
        u = (c[b] - 0.0) / 1.0
        assert e == [(1, float(np.float32((1 - u) * 0.5))), (0, float(np.float32((1 - u) * 0.5))), (2, float(np.float32(u)))], b
    # clamped: the first point's voice at and before it, the last point's at and after it -- their entries as they are
    got = S.morph_entries([(c[0], "1"), (c[1], "2:0.25,@v.npy:0.75")], 3, W, H, SR_HZ)
    assert got == [[(1, 1.0)], [(2, 0.25), ("v.npy", 0.75)], [(2, 0.25), ("v.npy", 0.75)]]
    got = S.morph_entries([(0.1, "1"), (0.2, "2"), (0.25, "3")], 3, W, H, SR_HZ)
    assert got[0] == [(1, 1.0)] and got[2] == [(3, 1.0)] and [s for s, _ in got[1]] == [1, 2]
    u = (c[1] - 0.1) / 0.1
    assert got[1] == [(1, float(np.float32(1 - u))), (2, float(np.float32(u)))]
    for bad in ([], [(1.0, "1"), (0.5, "2")], [(1.0, "1"), (1.0, "2")]):
        with pytest.raises(ValueError):
            S.morph_entries(bad, 2, W, H, SR_HZ)
    with pytest.raises(ValueError):
        S.morph_entries([(0.0, "x")], 2, W, H, SR_HZ)


def test_morph_and_voice_vectors_call_the_mix_once(monkeypatch, tmp_path, lib_built):
    """The native call stubbed: what it is handed -- the table with the vector files behind it, idx and w."""
    pred = UNetPredictor(32, num_labels=4)
    E = 128
    calls = []

    def stub(table, idx, w, out=None):
        calls.append((table.clone(), idx.clone(), w.clone()))
        return torch.zeros(idx.shape[0], table.shape[1])

    monkeypatch.setattr(S, "speaker_mix", stub)
    vec = np.arange(E, dtype=np.float32)
    path = str(tmp_path / "v.npy")
    S.save_voice(path, vec, dict(base_channels=32, steps=3))
    out = S.morph_vectors(pred, [(0.0, "1"), (1.0, f"@{path}:0.5,2:0.5")], 3, W, H, SR_HZ)
    assert tuple(out.shape) == (3, E) and len(calls) == 1
    table, idx, w = calls[0]
    assert tuple(table.shape) == (5, E) and torch.equal(table[:4], pred.class_embed.weight.detach()) and torch.equal(table[4], torch.from_numpy(vec))
    assert idx.dtype == torch.int32 and idx.tolist() == [[1, 4, 2]] * 3
    us = [(b * H + W / 2) / SR_HZ for b in range(3)]
    assert w.tolist() == [[float(np.float32(1 - u)), float(np.float32(u * 0.5)), float(np.float32(u * 0.5))] for u in us]
    # n = 1
    S.morph_vectors(pred, [(0.0, "1"), (1.0, "2")], 1, W, H, SR_HZ, label_offset=1)
    assert calls[1][1].tolist() == [[2, 3]] and calls[1][2].tolist() == [[float(np.float32(1 - us[0])), float(np.float32(us[0]))]]
    S.voice_vectors(pred, ["3", 0, "1:0.25,2:0.75", [(2, 2.0)]])
    assert calls[2][1].tolist() == [[3, -1], [0, -1], [1, 2], [2, -1]] and calls[2][2].tolist() == [[1.0, 0.0], [1.0, 0.0], [0.25, 0.75], [2.0, 0.0]]
    with pytest.raises(IndexError):
        S.voice_vectors(pred, ["4"])
    with pytest.raises(IndexError):
        S.voice_vectors(pred, ["3"], label_offset=1)
    S.save_voice(str(tmp_path / "short.npy"), vec[:64])
    with pytest.raises(ValueError, match="4 \\* base_channels"):
        S.voice_vectors(pred, [f"@{tmp_path / 'short.npy'}"])
    with pytest.raises(ValueError):
        S.voice_vectors(UNetPredictor(32), ["1"])


# ---------------------------------------------------------------- pseudo-voices
PSEUDO = {  # pseudo_voice(0, key, 251, 2): literals, so that a change of the rule -- or of a library under it -- shows
    "p225": "129:0.08539047837257385,168:0.9146094918251038",
    "p226": "219:0.5965254902839661,133:0.40347450971603394",
    "s5": "107:0.8312310576438904,174:0.16876892745494843",
}


def test_pseudo_voice():
    for key, want in PSEUDO.items():
        assert S.pseudo_voice(0, key, 251, 2) == want, key
    assert S.pseudo_voice(7, "p225", 251, 2) != PSEUDO["p225"]  # the seed matters
    assert S.pseudo_voice("0", "p225", 251, 2) == PSEUDO["p225"]  # ... through its text alone
    for k in (1, 3, 8):
        entries = S.parse_voice(S.pseudo_voice(1, "spk", 20, k))
        labels, weights = [l for l, _ in entries], np.array([w for _, w in entries], dtype=np.float32)
        assert len(set(labels)) == k and all(0 <= l < 20 for l in labels)
        assert (weights > 0).all() and abs(float(weights.astype(np.float64).sum()) - 1.0) < 1e-6
        assert all(float(np.float32(w)) == w for _, w in entries)  # rounded to float32 once, and written so that they read back
    assert S.parse_voice(S.pseudo_voice(1, "spk", 20, 1)) == [(S.parse_voice(S.pseudo_voice(1, "spk", 20, 3))[0][0], 1.0)]
    # exclude: never drawn, and the rest keep their order
    full = [l for l, _ in S.parse_voice(S.pseudo_voice(3, "x", 6, 6))]
    assert sorted(full) == list(range(6))
    for drop in (full[0], full[2]):
        got = [l for l, _ in S.parse_voice(S.pseudo_voice(3, "x", 6, 3, exclude=(drop,)))]
        assert got == [l for l in full if l != drop][:3]
    for bad in (dict(k=0), dict(k=9), dict(k=3, num_labels=2), dict(k=2, num_labels=3, exclude=(0, 1))):
        with pytest.raises(ValueError):
            S.pseudo_voice(0, "x", **dict(dict(num_labels=251, k=2), **bad))


def test_voice_files(tmp_path):
    vec = torch.randn(128, generator=torch.Generator().manual_seed(1))
    path = str(tmp_path / "sub.dir" / "v.npy")
    os.makedirs(os.path.dirname(path))
    S.save_voice(path, vec, dict(base_channels=32, steps=10, holdout_loss=0.25))
    got, meta = S.load_voice(path)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), vec.numpy().view(np.int32))
    assert meta == dict(base_channels=32, steps=10, holdout_loss=0.25, entries=128)
    assert json.load(open(str(tmp_path / "sub.dir" / "v.json"))) == meta
    os.remove(str(tmp_path / "sub.dir" / "v.json"))
    assert S.load_voice(path)[1] == {}
    for bad_path, bad_vec in ((str(tmp_path / "v.bin"), vec), (path, vec.double()), (path, vec.view(2, 64))):
        with pytest.raises(ValueError):
            S.save_voice(bad_path, bad_vec)
    np.save(str(tmp_path / "d.npy"), np.zeros(8))
    with pytest.raises(ValueError):
        S.load_voice(str(tmp_path / "d.npy"))


# ---------------------------------------------------------------- the scripts' flags
IO = ["--input-file", "in.wav", "ck.pt", "out.wav"]


@pytest.mark.parametrize("name", ["sample_vqvae", "sample_vqvae_uncond"])
def test_sampling_scripts_voice_flags(name, capsys):
    script = __import__(name)
    a = script.parse_args(IO + ["--label", "2"])
    assert (a.label, a.voice, a.voice_at) == (2, None, [])
    a = script.parse_args(IO + ["--voice", "3:0.7,1:0.3"])
    assert (a.label, a.voice, a.voice_at) == (None, "3:0.7,1:0.3", [])
    a = script.parse_args(IO + ["--whole-file", "--voice-at", "0:1", "--voice-at", "1.5:2:0.5,@v.npy:0.5"])
    assert (a.label, a.voice, a.voice_at) == (None, None, [(0.0, "1"), (1.5, "2:0.5,@v.npy:0.5")])
    for bad in ([], ["--label", "1", "--voice", "2"], ["--voice", "x"], ["--voice-at", "0:1", "--voice-at", "1:2"],  # no --whole-file
                ["--whole-file", "--voice-at", "0:1"], ["--whole-file", "--voice-at", "1:1", "--voice-at", "0.5:2"],
                ["--whole-file", "--voice-at", "0:1", "--voice-at", "0:2"], ["--whole-file", "--voice-at", "a:1", "--voice-at", "2:1"],
                ["--whole-file", "--voice-at", "0", "--voice-at", "2:1"], ["--whole-file", "--voice-at", "0:1", "--voice-at", "1:x"],
                ["--whole-file", "--label", "1", "--voice-at", "0:1", "--voice-at", "1:2"],
                ["--whole-file", "--voice", "1", "--voice-at", "0:1", "--voice-at", "1:2"]):
        with pytest.raises(SystemExit):
            script.parse_args(IO + bad)
    if name == "sample_vqvae":
        assert script.parse_args(IO + ["--voice", "1", "--sampler", "ddim", "--source-label", "2"]).source_label == 2  # stays an integer
        with pytest.raises(SystemExit):
            script.parse_args(IO + ["--voice", "1", "--sampler", "ddim", "--source-label", "2:0.5"])
    capsys.readouterr()


def test_other_scripts_voice_flags(capsys):
    import convert_dataset
    import enroll_speaker
    import eval_conversion

    base = ["m.pt", "data", "out"]
    a = convert_dataset.parse_args(base + ["--voice", "3:0.7,1:0.3"])
    assert (a.label, a.label_map, a.voice, convert_dataset.anonymize_of(a)) == (None, None, "3:0.7,1:0.3", None)
    a = convert_dataset.parse_args(base + ["--anonymize", "2"])
    assert (a.label, a.label_map, convert_dataset.voice_of(a), a.anonymize) == (None, None, None, 2)
    for bad in (["--voice", "x"], ["--voice", "1", "--label", "1"], ["--anonymize", "2", "--label", "1"], ["--anonymize", "2", "--voice", "1"],
                ["--anonymize", "2", "--label-map", "t.tsv"], ["--anonymize", "0"], ["--anonymize", "9"], []):
        with pytest.raises(SystemExit):
            convert_dataset.parse_args(base + bad)
    a = eval_conversion.parse_args(["vqvae.pt", "tones", "--voice", "3:0.7,1:0.3"])
    assert (a.voice, a.target) == ("3:0.7,1:0.3", "other")
    a = eval_conversion.parse_args(["vqvae.pt", "tones", "--voice", "2"])  # one label IS --target N
    assert (a.voice, a.target) == (None, 2)
    for bad in (["--voice", "x"], ["--voice", "1:0.5", "--target", "1"], ["--voice", "1:0.5", "--target", "same"]):
        with pytest.raises(SystemExit):
            eval_conversion.parse_args(["vqvae.pt", "tones"] + bad)
    with pytest.raises(SystemExit):
        eval_conversion.check_target("other", 3, "3:0.5,1:0.5")
    eval_conversion.check_target("other", 4, "3:0.5,@v.npy:0.5")
    st = eval_conversion.EvalState(classifier=True, voice=True)  # a blend is nobody's label: no target scores
    st.add_scores(8, 4, dict(code_match=[1], mcd=[1.0], lsd=[1.0], source_correct=[0]))
    assert "target_acc" not in st.log_dict() and "target_nll" not in st.log_dict() and "source_acc" in st.log_dict()
    with pytest.raises(ValueError):
        st.merge(eval_conversion.EvalState(classifier=True))

    pre = ["--pretrained-path", "m.pt"]
    a = enroll_speaker.parse_args(pre + ["--input-file", "a.wav", "--input-file", "b.wav", "--vector-out", "v.npy"])
    assert (a.data_dir, a.input_file, a.vector_out, a.vectors_out) == (None, ["a.wav", "b.wav"], "v.npy", None)
    a = enroll_speaker.parse_args(pre + ["speakers", "--vectors-out", "voices"])
    assert (a.data_dir, a.input_file, a.vector_out, a.vectors_out) == ("speakers", [], None, "voices")
    for bad in (["--input-file", "a.wav"], ["--input-file", "a.wav", "--vector-out", "v.bin"], ["speakers", "--input-file", "a.wav", "--vector-out", "v.npy"],
                ["--input-file", "a.wav", "--vector-out", "v.npy", "--uncond"], ["--input-file", "a.wav", "--vector-out", "v.npy", "--vectors-out", "d"],
                ["speakers", "--vector-out", "v.npy"], ["speakers", "--uncond", "--vectors-out", "d"], []):
        with pytest.raises(SystemExit):
            enroll_speaker.parse_args(pre + bad)
    clips = enroll_speaker.cut_clips([np.arange(10, dtype=np.float32), np.arange(3, dtype=np.float32), np.arange(4, dtype=np.float32)], 4)
    assert clips.tolist() == [[[0, 1, 2, 3]], [[4, 5, 6, 7]], [[0, 1, 2, 3]]]  # the partial clips dropped
    with pytest.raises(ValueError):
        enroll_speaker.cut_clips([np.arange(3, dtype=np.float32)], 4)  # fewer than one clip
    capsys.readouterr()


def test_label_maps_and_pairs_take_specs(tmp_path):
    import eval_parallel
    from vq_voice_swap_amd.corpus import read_label_map

    path = tmp_path / "map.tsv"
    path.write_text("s1\t2\ns2\t3:0.7,1:0.3\ns3\t@v.npy\n")
    assert read_label_map(str(path)) == {"s1": 2, "s2": "3:0.7,1:0.3", "s3": "@v.npy"}
    path.write_text("s1\t3:x\n")
    with pytest.raises(ValueError, match="map.tsv:1"):
        read_label_map(str(path))
    for rel in ("a.wav", "b.wav"):
        (tmp_path / rel).write_bytes(b"")
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("a.wav\tb.wav\t1\na.wav\tb.wav\t1:0.5,2:0.5\na.wav\tb.wav\t@v.npy\n")
    kw = dict(num_labels=3, limits=(1, 10), length=lambda p: 5)
    assert [p[2] for p in eval_parallel.read_pairs(str(pairs), str(tmp_path), **kw)] == [1, "1:0.5,2:0.5", "@v.npy"]
    for text in ("a.wav\tb.wav\t1:0.5,3:0.5\n", "a.wav\tb.wav\t1:\n"):
        pairs.write_text(text)
        with pytest.raises(ValueError, match="pairs.tsv:1"):
            eval_parallel.read_pairs(str(pairs), str(tmp_path), **kw)


def test_anonymize_plans_one_voice_per_directory(tmp_path, monkeypatch, capsys):
    """convert_dataset.main --anonymize 2 with the model and the conversion stubbed: the tsv, and what every file is converted to."""
    import convert_dataset
    from vq_voice_swap_amd.audio import ChunkWriter
    from vq_voice_swap_amd.corpus import read_label_map

    data = tmp_path / "data"
    for rel, n in (("s1/a.wav", 800), ("s1/c/b.wav", 4000), ("s2/a.wav", 300), ("s2/b.wav", 300)):
        os.makedirs(data / os.path.dirname(rel), exist_ok=True)
        w = ChunkWriter(str(data / rel), 16000)
        w.write(torch.zeros(n).numpy())
        w.close()

    class Model:
        num_labels = 5

        def to(self, device):
            return self

        def eval(self):
            return self

        def set_precision(self, precision):
            return self

    seen = {}

    def convert_pack(args, model, enc_pred, device, files, labels, pack, window, hop):
        for i in pack:
            seen[files[i][0]] = labels[i]
        return len(pack), 0, 0, 0, 1

    monkeypatch.setattr(convert_dataset.VQVAE, "load", staticmethod(lambda path: Model()))
    monkeypatch.setattr(convert_dataset, "local_device", lambda why: torch.device("cpu"))
    monkeypatch.setattr(convert_dataset, "convert_pack", convert_pack)
    out = tmp_path / "out"
    argv = ["m.pt", str(data), str(out), "--anonymize", "2", "--seed", "4", "--window-seconds", "0.128", "--overlap-seconds", "0.032"]
    convert_dataset.main(argv)
    want = {d: S.pseudo_voice(4, d, 5, 2) for d in ("s1", "s2")}
    assert want["s1"] != want["s2"]
    assert (out / "pseudo_voices.tsv").read_text() == "".join(f"{d}\t{spec}\n" for d, spec in want.items())
    assert read_label_map(str(out / "pseudo_voices.tsv")) == want  # a label map the script reads back
    assert seen == {os.path.join("s1", "a.wav"): want["s1"], os.path.join("s1", "c", "b.wav"): want["s1"],
                    os.path.join("s2", "a.wav"): want["s2"], os.path.join("s2", "b.wav"): want["s2"]}
    # packing does not enter: the same plan under another budget; guidance counts the speakers without the null label
    seen.clear()
    convert_dataset.main(argv + ["--pack-windows", "1", "--guide-label-scale", "2"])
    assert seen[os.path.join("s2", "b.wav")] == S.pseudo_voice(4, "s2", 4, 2)
    with pytest.raises(SystemExit):
        convert_dataset.main(argv[:3] + ["--anonymize", "6"] + argv[5:])  # more speakers per voice than the model has
    capsys.readouterr()


# ---------------------------------------------------------------- the library's surface
def test_entry_points_are_declared_exported_and_bound(lib_built):
    header = " ".join(open(os.path.join(ROOT, "include", "vqvs.h")).read().split())
    want = {"vqvs_unet_forward_vec": ["vqvs_model* m", "const float* d_x", "const float* d_ts", "const float* d_cond", "const float* d_vec", "float* d_out",
                                      "int B", "int T", "void* stream"],
            "vqvs_speaker_mix": ["const float* d_table", "int K", "int E", "const int32_t* d_idx", "const float* d_w", "int J", "float* d_out", "int B",
                                 "void* stream"]}
    for name, args in want.items():
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl, f"include/vqvs.h does not declare {name}"
        assert [a.strip() for a in decl.group(1).split(",")] == args
        assert name in _native.EXPORTS and hasattr(lib_built, name) and len(getattr(lib_built, name).argtypes) == len(args)
    assert "speaker_kernels.hip" in open(os.path.join(ROOT, "vq_voice_swap_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_arguments_without_a_device(lib_built):
    L = lib_built
    table = (C.c_float * 64)()
    out = (C.c_float * 64)()
    idx, w = (C.c_int32 * 16)(), (C.c_float * 16)()
    p = lambda b, off=0: C.c_void_p(C.addressof(b) + off)  # noqa: E731
    ok = dict(table=p(table), K=4, E=16, idx=p(idx), w=p(w), J=2, out=p(out), B=4)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_speaker_mix(a["table"], a["K"], a["E"], a["idx"], a["w"], a["J"], a["out"], a["B"], None)

    for bad in (dict(table=None), dict(idx=None), dict(w=None), dict(out=None), dict(K=0), dict(E=0), dict(B=0), dict(K=-1), dict(J=0), dict(J=17),
                dict(out=p(table)), dict(out=p(table, 4 * 63)), dict(out=p(idx)), dict(out=p(w, 4))):
        assert call(**bad) == -1 and L.vqvs_last_error(), bad
    x = p(out)
    assert L.vqvs_unet_forward_vec(None, x, x, None, x, x, 1, 64, None) == -1


# ---------------------------------------------------------------- the restatement itself
def test_mix_ref_is_the_ordered_float32_sum():
    """Against float64 on well-scaled inputs (1e-6 relative: it is a float32 sum), and the corner cases by hand."""
    rng = np.random.RandomState(0)
    table, w = rng.randn(5, 12).astype(np.float32), rng.randn(3, 4).astype(np.float32)
    idx = rng.randint(0, 5, (3, 4)).astype(np.int32)
    idx[1, 0] = idx[1, 2] = -1
    got = SR.mix_ref(table, idx, w)
    want = np.zeros((3, 12))
    for b in range(3):
        for j in range(4):
            if idx[b, j] >= 0:
                want[b] += float(w[b, j]) * table[idx[b, j]].astype(np.float64)
    assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-5
    one = SR.mix_ref(table, np.array([[-1, 3, -1]]), np.array([[5.0, 1.0, 7.0]], dtype=np.float32))
    assert np.array_equal(one.view(np.int32), table[3:4].view(np.int32))  # w = 1: the row itself
    neg = SR.mix_ref(-np.zeros((1, 4), dtype=np.float32), np.array([[0]]), np.ones((1, 1), dtype=np.float32))
    assert np.signbit(neg).all()  # nothing was added to a +0
    assert not SR.mix_ref(table, np.array([[-1, -1]]), np.ones((1, 2), dtype=np.float32)).any()  # no used slot: zeros
    assert np.array_equal(SR.mix_ref(table, np.array([[9]]), np.ones((1, 1), dtype=np.float32)), table[4:5])  # clamped to the last row
    # the order matters, which is why it is fixed: (big + small) - big loses the small term
    t3 = np.array([[1e8], [1.0], [-1e8]], dtype=np.float32)
    a = SR.mix_ref(t3, np.array([[0, 1, 2]]), np.ones((1, 3), dtype=np.float32))
    b = SR.mix_ref(t3, np.array([[0, 2, 1]]), np.ones((1, 3), dtype=np.float32))
    assert a[0, 0] == 0.0 and b[0, 0] == 1.0
    for unused in ("none", "some", "all"):
        table, idx, w = SR.mix_case(4, 6, 5, 16, 3, unused)
        assert np.isfinite(SR.mix_ref(table, idx, w)).all()
        assert (idx[0] < 0).all() == (unused == "all") and ((idx < 0).any() == (unused != "none"))
