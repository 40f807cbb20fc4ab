"""Drop-in ``KeyDataset`` whose CQT stage runs on the GPU.

Keeps the reference's dataset surface (KeyDataset.py:32-264): ``KeyDataset(genre, opt)``,
``import_data(*loaders)``, ``len()``, ``ds[i]`` -> the item dict of KeyDataset.py:242-256 with the
same keys, dtypes and zero padding to ``seq_length_max``; loaders expose ``name``,
``get_filenames()`` and ``get_all(file, pitch_shift, genre, opt, multi_scale)``.

With ``opt.local`` (per-frame key tracking) every label tensor of a clip with T CQT frames is its
row repeated ``T - (loc_window_size * frames - 1)`` times (KeyDataset.py:345-348, 457-465: the
non-Winterreise path), and ``ds[i]`` zero-pads the mel and every label tensor to
``seq_length_max`` rows with ``seq_length = T`` (KeyDataset.py:225-241).  Winterreise's local-key
segment annotations are not built (annotation parsing is out of scope, see below).

What differs, on purpose: the reference computes one CQT per file on a CPU thread inside
``get_all`` (KeyDataset.py:488-495) and caches it on disk.  Here loaders hand over *waveforms*
and ``import_data`` batches clips of equal length through ``ake_cqt_logmag_f32``; nothing is
cached on disk.  File-system loaders for the 14 public datasets, annotation parsing and audio
decoding (KeyDataset.py:268-466, 514-1233) are out of scope: ``SyntheticSineMixLoader`` and
``WaveformLoader`` supply clips instead.
"""
from __future__ import annotations

import random
from collections import defaultdict

import numpy as np
import torch

from . import synthetic
from .cqt import WHOLE_SONG_FRAMES, get_any_hop_plan, get_plan, hop_for, hop_for_window, whole_song_frames

SIGNATURE = [n + " minor" for n in ("C", "Db", "D", "Eb", "E", "F", "Gb", "G", "Ab", "A", "Bb", "B")] + \
            [n + " major" for n in ("C", "Db", "D", "Eb", "E", "F", "Gb", "G", "Ab", "A", "Bb", "B")]   # KeyDataset.py:524-527
_ENHARMONIC = {"C#": "Db", "D#": "Eb", "F#": "Gb", "G#": "Ab", "A#": "Bb", "Cb": "B", "E#": "F", "B#": "C", "Fb": "E"}


def signature_id(key_name: str) -> int:
    """'F# minor' / 'Bb major' -> index into the 24-way ``signature`` list (0..11 minor, 12..23 major)."""
    tonic, mode = key_name.strip().split()
    tonic = _ENHARMONIC.get(tonic, tonic)
    return SIGNATURE.index(f"{tonic} {mode}")


def labels_for_signature(sig: int, genre_id: int | None, genre_flag: bool):
    """Label tensors of KeyDataset.py:443-454 for key ``sig``; genre is zeros(8) when the flag is off (:476)."""
    key_labels = torch.from_numpy(synthetic.key_pitch_classes(sig))
    key_signature_id = torch.nn.functional.one_hot(torch.tensor(sig), 24).float()
    tonic = torch.nn.functional.one_hot(torch.tensor(sig % 12), 12).float()
    if genre_flag:
        genre = torch.zeros(synthetic.N_GENRES)
        if genre_id is not None and genre_id >= 0:
            genre[genre_id] = 1.0
    else:
        genre = torch.zeros(8)
    return key_labels, key_signature_id, genre, tonic


def local_labels(labels, n_frames: int, opt, clip=None):
    """--local per-frame labels (KeyDataset.py:345-348, 457-465): each (C,) label tensor of ``labels`` -> its row repeated over the
    clip's ``time_length = n_frames - (loc_window_size * frames - 1)`` rows, (time_length, C).  A clip shorter than one local window
    (time_length < 1) is refused: the reference gives it an empty label tensor and a NaN loss."""
    span = getattr(opt, "loc_window_size", 10) * getattr(opt, "frames", 5)
    rows = n_frames - (span - 1)
    if rows < 1:
        raise ValueError(f"--local: clip {clip!r} has {n_frames} CQT frames, fewer than the {span} of one local window "
                         f"(loc_window_size * frames): it has no frame to label")
    return tuple(t.reshape(1, -1).repeat(rows, 1) for t in labels)


def pad_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    """(r, C) -> (rows, C), zeros after the first r rows (KeyDataset.py:228-233)."""
    return torch.cat((t, torch.zeros([rows - t.shape[0], t.shape[1]], dtype=t.dtype)), dim=0)


class DatasetLoader:
    """Loader protocol (KeyDataset.py:268-313): subclasses supply clips and key names."""

    def __init__(self, dataset_loc=None):
        self.name = None
        self.dataset_loc = dataset_loc
        self.size = -1

    def get_filenames(self):
        raise NotImplementedError("The standard Dataset Loader has no allocated Dataset")

    def get_size(self):
        return self.size

    def get_waveform(self, file_id):
        """-> (waveform float32 (n,), sample_rate); an int16 array is 16-bit PCM (sample / 32768, ``ake_amd.pcm16_to_float``)"""
        raise NotImplementedError

    def get_key_signature_id(self, file_id) -> int:
        raise NotImplementedError

    def get_genre_id(self, file_id):
        return None

    def get_all(self, file_id, pitch_shift, genre, opt, multi_scale=False):
        """Single-clip path with the reference's return order (KeyDataset.py:469-509)."""
        wav, sr = self.get_waveform(file_id)
        mel = cqt_features(torch.as_tensor(wav)[None], sr, opt)[0]
        key_labels, key_signature_id, g, tonic = labels_for_signature(self.get_key_signature_id(file_id), self.get_genre_id(file_id), genre)
        return mel.reshape(1, mel.shape[0], mel.shape[1]).double().cpu(), key_labels, key_signature_id, g, tonic


class SyntheticSineMixLoader(DatasetLoader):
    """Seeded sine-mix clips (synthetic.py): clip i has key ``i % 24`` and genre ``i % 11``."""

    def __init__(self, n_clips, first=0, n_samples=synthetic.N_SAMPLES, sample_rate=synthetic.SR, name="Synthetic SineMix"):
        super().__init__(None)
        self.name = name
        self.size = n_clips
        self.first, self.n_samples, self.sample_rate = first, n_samples, sample_rate

    def get_filenames(self):
        return list(range(self.first, self.first + self.size))

    def get_waveform(self, file_id):
        return synthetic.make_clip(int(file_id), self.n_samples, self.sample_rate)[0], self.sample_rate

    def get_key_signature_id(self, file_id):
        return int(file_id) % 24

    def get_genre_id(self, file_id):
        return int(file_id) % synthetic.N_GENRES


class WaveformLoader(DatasetLoader):
    """In-memory clips: ``waveforms`` list of 1-D arrays, ``keys`` like 'A minor', optional genre ids."""

    def __init__(self, name, waveforms, keys, sample_rate, genres=None):
        super().__init__(None)
        self.name, self.sample_rate = name, sample_rate
        self.waveforms, self.keys, self.genres = waveforms, keys, genres
        self.size = len(waveforms)

    def get_filenames(self):
        return list(range(self.size))

    def get_waveform(self, file_id):
        wav = np.asarray(self.waveforms[file_id])
        if wav.dtype == np.int16:                                    # 16-bit PCM stays PCM: import_data runs the PCM CQT on it
            return wav, self.sample_rate
        return wav.astype(np.float32, copy=False), self.sample_rate

    def get_key_signature_id(self, file_id):
        k = self.keys[file_id]
        return k if isinstance(k, int) else signature_id(k)

    def get_genre_id(self, file_id):
        return None if self.genres is None else self.genres[file_id]


def cqt_features(waveforms: torch.Tensor, rate: int, opt, lengths=None) -> torch.Tensor:
    """(B, n) waveforms -> log-CQT (B, 36*octaves, T) float32 on the GPU (KeyDataset.py:485-499); ``lengths``: samples per row of
    a ragged batch (clip i then has ``1 + lengths[i] // hop`` frames, zeros after them).

    ``opt.frames == 0`` (whole songs, KeyDataset.py:485-503, 212-215): clip i gets its own hop ``n_i // opt.window_size + 1``, hence
    ``T_i = 1 + n_i // hop_i <= window_size`` frames, cropped to ``window_size`` and zero-padded to 592; the result has
    ``F = max(min(window_size, max T_i), 592)`` frames, clip i's first T_i of them its own, zeros after them."""
    frames = getattr(opt, "frames", 5)
    if getattr(opt, "only_semitones", False) or getattr(opt, "multi_scale", False):
        raise NotImplementedError("--only_semitones / --multi_scale CQTs are not built (SURVEY.md section 2.1)")
    # opt.cqt_q_mode (not a reference option): 1 selects librosa <= 0.9's filter Q, see ake_amd.cqt.get_plan
    q_mode, n_bins = int(getattr(opt, "cqt_q_mode", 0)), 36 * getattr(opt, "octaves", 8)
    if frames <= 0:
        return whole_song_cqt(waveforms, rate, n_bins, getattr(opt, "window_size", WHOLE_SONG_FRAMES), lengths, q_mode)
    plan = get_plan(rate, hop_for(rate, frames), n_bins, 36, q_mode=q_mode)
    return plan.logmag(waveforms, lengths=lengths)


def whole_song_cqt(waveforms: torch.Tensor, rate: int, n_bins: int = 288, window_size: int = WHOLE_SONG_FRAMES, lengths=None,
                   q_mode: int = 0) -> torch.Tensor:
    """--frames 0 front end (see cqt_features): one ragged launch with a hop per clip."""
    if waveforms.dim() == 1:
        waveforms = waveforms[None]
    B, n = waveforms.shape
    lens_host = torch.full((B,), n, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths).reshape(-1).to("cpu", torch.int64)
    T_max = int((1 + lens_host // hop_for_window(lens_host, window_size)).max())
    F = max(min(window_size, T_max), WHOLE_SONG_FRAMES)      # (every T_i <= window_size: the crop of KeyDataset.py:501-503 never cuts)
    plan = get_any_hop_plan(rate, n_bins, 36, q_mode=q_mode)
    lens = (lens_host if lengths is None else torch.as_tensor(lengths).reshape(-1)).to(plan.device, torch.int64)
    hops = hop_for_window(lens, window_size).to(torch.int32)                      # computed on the device
    return plan.logmag_hops(waveforms, hops, lens if lengths is not None else None, out_frames=F)


class KeyDataset:

    def __init__(self, genre, opt, cqt_batch=64):
        self.datasets = {}
        self.filenames = []
        self.genre = genre
        self.mel, self.mel2 = {}, {}
        self.key_labels, self.key_signature_id, self.genre_labels, self.tonic_labels = {}, {}, {}, {}
        self.opt = opt
        self.seq_length_max = 0
        self.cqt_batch = cqt_batch
        self.local = bool(getattr(opt, "local", False))
        if self.local and getattr(opt, "frames", 5) <= 0:
            raise ValueError("--local needs --frames > 0: its per-frame labels are counted in local windows of loc_window_size * frames "
                             "CQT frames")

    def __len__(self):
        return len(self.filenames)

    def load_files(self, *dataset_loaders):
        self.filenames = []
        for loader in dataset_loaders:
            if not isinstance(loader, DatasetLoader):
                continue
            for f in loader.get_filenames():
                self.filenames.append((f, loader.name, torch.tensor(0)))             # KeyDataset.py:64-76

    def load_dataset_handler(self, *dataset_loaders):
        for loader in dataset_loaders:
            if isinstance(loader, DatasetLoader):
                self.datasets[loader.name] = loader

    def import_data(self, *dataset_loaders, shuffle=True):
        self.load_files(*dataset_loaders)
        self.load_dataset_handler(*dataset_loaders)
        if shuffle:
            random.shuffle(self.filenames)                                            # KeyDataset.py:97
        self.store_content()
        self.find_longest_seq()
        print("Length of Data: " + str(len(self.mel)))

    def store_content(self):
        """All clips -> CQT on the GPU, batched by sample rate: clips of different lengths share a launch (ragged batch, sorted by
        length so that a batch pads little); every clip keeps its own frame count; labels per clip (KeyDataset.py:121-138)."""
        groups = defaultdict(list)
        waves = {}
        for idx, (f, dname, _) in enumerate(self.filenames):
            wav, sr = self.datasets[dname].get_waveform(f)
            wav = torch.as_tensor(wav)
            pcm = wav.dtype == torch.int16                           # 16-bit PCM clips batch among themselves, through the PCM CQT
            waves[idx] = (wav if pcm else wav.to(torch.float32)).reshape(-1)
            groups[(sr, pcm)].append(idx)
        frames = getattr(self.opt, "frames", 5)
        window = getattr(self.opt, "window_size", WHOLE_SONG_FRAMES)
        for (sr, pcm), idxs in groups.items():
            idxs = sorted(idxs, key=lambda i: waves[i].numel())
            # frames kept per clip: 1 + n // hop; --frames 0: max(T_i, 592) (KeyDataset.py:212-215)
            keep = (lambda n: whole_song_frames(n, window)) if frames <= 0 else (lambda n, hop=hop_for(sr, frames): 1 + n // hop)
            for s in range(0, len(idxs), self.cqt_batch):
                part = idxs[s:s + self.cqt_batch]
                lens = [waves[i].numel() for i in part]
                if min(lens) == max(lens):
                    mel = cqt_features(torch.stack([waves[i] for i in part]), sr, self.opt)
                else:
                    batch = torch.zeros((len(part), max(lens)), dtype=torch.int16 if pcm else torch.float32)
                    for j, i in enumerate(part):
                        batch[j, :lens[j]] = waves[i]
                    mel = cqt_features(batch, sr, self.opt, lengths=torch.tensor(lens, dtype=torch.int64))
                mel = mel.double().cpu()                                               # .double(): KeyDataset.py:509
                for j, i in enumerate(part):
                    self.mel[str(i)] = mel[j:j + 1, :, :keep(lens[j])].clone()          # (1, bins, T_i)
                    self.mel2[str(i)] = None
        self.store_labels()
        print("done", flush=True)

    def store_labels(self):
        """Labels of every clip (KeyDataset.py:441-467); with --local per frame of its stored mel (local_labels)."""
        for idx, (f, dname, _) in enumerate(self.filenames):
            ld = self.datasets[dname]
            labels = labels_for_signature(ld.get_key_signature_id(f), ld.get_genre_id(f), self.genre)
            if self.local:
                labels = local_labels(labels, self.mel[str(idx)].shape[2], self.opt, clip=f"{dname}/{f}")
            kl, ks, g, t = labels
            self.key_labels[str(idx)], self.key_signature_id[str(idx)] = kl, ks
            self.genre_labels[str(idx)], self.tonic_labels[str(idx)] = g, t

    def find_longest_seq(self):
        for i in range(len(self.mel)):                                                # KeyDataset.py:113-119
            self.seq_length_max = max(self.seq_length_max, self.mel[str(i)].shape[2])
        print("Max. Seq. Length: " + str(self.seq_length_max))

    def __getitem__(self, idx):
        mel = self.mel[str(idx)]
        if self.local:                                                                  # KeyDataset.py:224-241
            rows = self.seq_length_max
            padded = torch.cat((mel, torch.zeros([mel.shape[0], mel.shape[1], rows - mel.shape[2]], dtype=mel.dtype)), dim=2)
            return {"mel": padded, "key_labels": pad_rows(self.key_labels[str(idx)], rows),
                    "tonic_labels": pad_rows(self.tonic_labels[str(idx)], rows),
                    "key_signature_id": pad_rows(self.key_signature_id[str(idx)], rows),
                    "genre": pad_rows(self.genre_labels[str(idx)], rows), "seq_length": mel.shape[2]}
        if getattr(self.opt, "frames", 5) <= 0:                                          # KeyDataset.py:257-262: no seq_length, no padding
            return {"mel": mel, "key_labels": self.key_labels[str(idx)], "tonic_labels": self.tonic_labels[str(idx)],
                    "key_signature_id": self.key_signature_id[str(idx)], "genre": self.genre_labels[str(idx)]}
        seq_length = mel.shape[2]
        pad = self.seq_length_max - seq_length
        padded = torch.cat((mel, torch.zeros([mel.shape[0], mel.shape[1], pad], dtype=mel.dtype)), dim=2)   # KeyDataset.py:243-245
        return {"mel": padded, "key_labels": self.key_labels[str(idx)], "tonic_labels": self.tonic_labels[str(idx)],
                "key_signature_id": self.key_signature_id[str(idx)], "genre": self.genre_labels[str(idx)],
                "seq_length": seq_length}                                              # KeyDataset.py:249-256
