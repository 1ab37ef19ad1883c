"""
Evaluation data: the reference's `create_data_loader` call surface (reference vq_voice_swap/dataset.py:12-151) for the
denoising-loss evals -- the synthetic "tones" set and a LibriSpeech-layout directory of WAV files read through
`audio.ChunkReader`.

This module imports neither the native library nor anything that opens a device: with `num_workers > 0` the loader's workers
are SPAWNED (never forked from a process that may hold a HIP context) and only ever run the code below.
"""

from __future__ import annotations

import json
import os
import struct
from typing import Dict, Iterator, List, Optional, Tuple, Union

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset, Sampler

from .audio import ChunkReader, encode_from_linear

DURATION_SLACK = 0.05  # seconds taken off a file's stated duration before it is cut into windows (reference dataset.py:9,86)
TONE_HZ = (300, 500, 1000)
TONE_PHASES, TONE_SAMPLES, TONE_RATE = 10, 64000, 16000


class AudioFormatError(ValueError):
    pass


class ToneDataset(Dataset):
    """Three "speakers" of 300 / 500 / 1000 Hz, ten phase shifts each: item i is speaker i % 3 at phase (i // 3) / 10 s,
    sin(2 pi f (n / 16000 + phase)) for n < 64000.  The argument is formed in float64 (the reference forms it in float32, where it
    is good to ~2e-3 rad at the far end of a clip)."""

    def __init__(self, encoding: str = "linear"):
        self.encoding = encoding
        self.speaker_ids = list(TONE_HZ)
        self._time = np.arange(TONE_SAMPLES, dtype=np.float64) / TONE_RATE

    def __len__(self) -> int:
        return len(self.speaker_ids) * TONE_PHASES

    def __getitem__(self, index: int) -> Dict[str, Union[int, np.ndarray]]:
        if not 0 <= index < len(self):
            raise IndexError(index)
        speaker, shift = index % len(self.speaker_ids), index // len(self.speaker_ids)
        wave = np.sin((self._time + shift / TONE_PHASES) * (2 * np.pi * self.speaker_ids[speaker])).astype(np.float32)
        return {"label": speaker, "samples": encode_from_linear(wave, self.encoding)}


def wav_duration(path: str) -> float:
    """Seconds of audio in a RIFF/WAVE file, from its header alone."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise AudioFormatError(f"{path}: not a RIFF/WAVE file")
        byte_rate = None
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                raise AudioFormatError(f"{path}: WAVE file without fmt / data chunk")
            cid, size = hdr[:4], struct.unpack("<I", hdr[4:])[0]
            if cid == b"fmt ":
                body = f.read(size + (size & 1))
                if len(body) < 16:
                    raise AudioFormatError(f"{path}: truncated WAVE fmt chunk")
                _, ch, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                byte_rate = rate * ch * (bits // 8)
            elif cid == b"data":
                if not byte_rate:
                    raise AudioFormatError(f"{path}: WAVE data chunk before a usable fmt chunk")
                left = os.fstat(f.fileno()).st_size - f.tell()
                return min(size, left) / byte_rate
            else:
                f.seek(size + (size & 1), os.SEEK_CUR)


def _scan(directory: str, seen_flac: List[str]) -> Dict[str, Union[dict, float]]:
    out = {}
    for name in sorted(os.listdir(directory)):
        path = os.path.join(directory, name)
        if name.startswith("."):
            continue
        if os.path.isdir(path):
            sub = _scan(path, seen_flac)
            if sub:
                out[name] = sub
        elif name.lower().endswith(".wav"):
            out[name] = float(wav_duration(path))
        elif name.lower().endswith(".flac"):
            seen_flac.append(path)
    return out


def build_file_index(directory: str) -> Dict[str, dict]:
    """{speaker directory: {sub-directory: {... file name: seconds}}} of every WAV file below the speaker directories."""
    flac: List[str] = []
    index = {}
    for name in sorted(os.listdir(directory)):  # (files directly in `directory` belong to no speaker)
        if not name.startswith(".") and os.path.isdir(os.path.join(directory, name)):
            sub = _scan(os.path.join(directory, name), flac)
            if sub:
                index[name] = sub
    if not index:
        if flac:
            raise AudioFormatError(f"{directory} holds only FLAC audio (e.g. {flac[0]}): there is no FLAC decoder here; convert the "
                                   "set to WAV, keeping the directory layout (speaker / chapter / file)")
        raise AudioFormatError(f"{directory}: no WAV files under any speaker directory")
    return index


class SpeakerWindows(Dataset):
    """Windows of `window_duration` seconds every `window_spacing` seconds over each file of a LibriSpeech-layout tree: the
    top-level directory names the speaker, a speaker's label is its position in sorted order.  A file shorter than a window
    gives one zero-padded window.  The file index (durations) is cached as index.json in the directory."""

    def __init__(self, directory: str, encoding: str = "linear", window_duration: float = 4.0, window_spacing: float = 0.2,
                 sample_rate: int = 16000):
        self.directory, self.encoding, self.sample_rate = directory, encoding, sample_rate
        self.window_samples = int(sample_rate * window_duration)
        self.spacing_samples = int(sample_rate * window_spacing)
        if self.window_samples < 1 or self.spacing_samples < 1:
            raise ValueError("window_duration and window_spacing must cover at least one sample")
        index_path = os.path.join(directory, "index.json")
        if os.path.exists(index_path):
            with open(index_path, "rt") as f:
                self.index = json.load(f)
        else:
            self.index = build_file_index(directory)
            with open(index_path, "wt") as f:
                json.dump(self.index, f)
        self.speaker_ids = sorted(self.index.keys())
        self.data: List[Tuple[int, str, int]] = []  # (label, path, offset in samples)
        for label, speaker in enumerate(self.speaker_ids):
            self._add(label, os.path.join(directory, speaker), self.index[speaker])

    def _add(self, label: int, path: str, node: dict) -> None:
        for name, item in node.items():
            sub = os.path.join(path, name)
            if isinstance(item, dict):
                self._add(label, sub, item)
                continue
            total = int(self.sample_rate * (float(item) - DURATION_SLACK))
            offsets = range(0, total - self.window_samples, self.spacing_samples) if self.window_samples < total else (0,)
            self.data.extend((label, sub, off) for off in offsets)

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, index: int) -> Dict[str, Union[int, np.ndarray]]:
        label, path, offset = self.data[index]
        if path.lower().endswith(".flac"):
            raise AudioFormatError(f"{path}: the index lists FLAC audio and there is no FLAC decoder here; convert the set to WAV")
        reader = ChunkReader(path, self.sample_rate, encoding=self.encoding)
        try:
            if offset:
                reader.read(offset)
            chunk = reader.read(self.window_samples)
        finally:
            reader.close()
        out = np.zeros(self.window_samples, dtype=np.float32)
        if chunk is not None:
            out[:len(chunk)] = chunk
        return {"label": label, "samples": out}


class ShardedBatches(Sampler):
    """Index batches of a (seeded) permutation, incomplete last batch dropped; shard (rank, world) yields batches rank, rank +
    world, ... of that one list, so every rank count walks the same batches."""

    def __init__(self, n: int, batch_size: int, shuffle: bool = True, seed: Optional[int] = None, rank: int = 0, world: int = 1):
        self.n, self.batch_size, self.shuffle, self.seed, self.rank, self.world = n, batch_size, shuffle, seed, rank, world

    def batches(self) -> List[List[int]]:
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(int(self.seed) if self.seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item()))
            order = torch.randperm(self.n, generator=g).tolist()
        else:
            order = list(range(self.n))
        full = [order[i:i + self.batch_size] for i in range(0, self.n - self.batch_size + 1, self.batch_size)]
        return full[self.rank::self.world]

    def __iter__(self) -> Iterator[List[int]]:
        return iter(self.batches())

    def __len__(self) -> int:
        total = self.n // self.batch_size
        return len(range(self.rank, total, self.world))


def create_data_loader(directory: str, batch_size: int, encoding: str = "linear", num_workers: int = 0, *, shuffle: bool = True,
                       seed: Optional[int] = None, rank: int = 0, world: int = 1, **dataset_kwargs) -> Tuple[DataLoader, int]:
    """(loader, num_labels); batches are {"label": int64 [N], "samples": float32 [N, T]}.  `directory` is "tones" or a
    LibriSpeech-layout tree of WAV files (`window_duration`, `window_spacing`, `sample_rate` go to `SpeakerWindows`).  Shuffled
    with the last incomplete batch dropped, as the reference's loader; `seed` fixes the order, (rank, world) shards the batches."""
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    dataset = ToneDataset(encoding=encoding, **dataset_kwargs) if directory == "tones" else SpeakerWindows(directory, encoding=encoding, **dataset_kwargs)
    sampler = ShardedBatches(len(dataset), batch_size, shuffle=shuffle, seed=seed, rank=rank, world=world)
    loader = DataLoader(dataset, batch_sampler=sampler, num_workers=num_workers,
                        multiprocessing_context="spawn" if num_workers > 0 else None)
    return loader, len(dataset.speaker_ids)
