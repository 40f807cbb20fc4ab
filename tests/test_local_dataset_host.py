"""HOST: KeyDataset with opt.local -- per-frame labels and the padded items (reference KeyDataset.py:345-348, 457-465, 225-241),
checked against a restatement of those lines.  The CQT is not needed: the mels are stored by hand, as import_data would store them."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import ake_amd
from ake_amd.KeyDataset import labels_for_signature, local_labels, pad_rows

SPAN = 50                                  # loc_window_size * frames of the reference's defaults


def local_opt(**kw):
    o = dict(local=True, frames=5, loc_window_size=10, octaves=8, window_size=592, multi_scale=False, only_semitones=False)
    o.update(kw)
    return Namespace(**o)


def reference_item(mel, key_labels, key_signature_id, genre, tonic_label, opt, seq_length_max):
    """KeyDataset.py:345-348 and 457-465 (non-Winterreise path), then 225-241, with torch in place of tf."""
    time_length = mel.shape[2] - (opt.loc_window_size * opt.frames - 1)
    key_signature_id = key_signature_id.reshape(1, key_signature_id.shape[0]).repeat(time_length, 1)
    key_labels = key_labels.reshape(1, key_labels.shape[0]).repeat(time_length, 1)
    tonic_label = tonic_label.reshape(1, tonic_label.shape[0]).repeat(time_length, 1)
    genre = genre.reshape(1, genre.shape[0]).repeat(time_length, 1)
    seq_length = mel.shape[2]
    padded_seq_length = seq_length_max
    pad = lambda t: torch.cat((t, torch.zeros([padded_seq_length - t.shape[0], t.shape[1]])), dim=0)
    return {"mel": torch.cat((mel, torch.zeros([mel.shape[0], mel.shape[1], padded_seq_length - mel.shape[2]], dtype=mel.dtype)), dim=2),
            "key_labels": pad(key_labels), "tonic_labels": pad(tonic_label), "key_signature_id": pad(key_signature_id),
            "genre": pad(genre), "seq_length": seq_length}


def build(genre, frames_per_clip, keys, genres=None, opt=None):
    """A --local KeyDataset whose clips have the given CQT frame counts (mels stored directly; labels as import_data makes them)."""
    opt = opt or local_opt()
    ds = ake_amd.KeyDataset(genre, opt)
    loader = ake_amd.WaveformLoader("clips", [np.zeros(8, np.float32)] * len(keys), keys, 22050, genres=genres)
    ds.load_files(loader)
    ds.load_dataset_handler(loader)
    g = torch.Generator().manual_seed(1)
    for i, T in enumerate(frames_per_clip):
        ds.mel[str(i)] = torch.rand((1, 288, T), generator=g, dtype=torch.float64)
        ds.mel2[str(i)] = None
    ds.store_labels()
    ds.find_longest_seq()
    return ds, loader


@pytest.mark.parametrize("genre", [False, True])
def test_items_match_the_reference(genre):
    frames = [61, 101, 156, 50]
    keys = ["A minor", "C major", "F# minor", "Bb major"]
    ds, loader = build(genre, frames, keys, genres=[3, None, 7, 10])
    assert ds.seq_length_max == 156 and len(ds) == 4
    for i, T in enumerate(frames):
        item = ds[i]
        labels = labels_for_signature(loader.get_key_signature_id(i), loader.get_genre_id(i), genre)
        want = reference_item(ds.mel[str(i)], *labels, ds.opt, 156)
        assert list(item) == list(want)
        assert item["seq_length"] == T == want["seq_length"]
        rows = T - (SPAN - 1)
        for k in ("mel", "key_labels", "tonic_labels", "key_signature_id", "genre"):
            assert item[k].dtype == want[k].dtype and torch.equal(item[k], want[k]), (i, k)
        width = {"key_labels": 12, "tonic_labels": 12, "key_signature_id": 24, "genre": 11 if genre else 8}
        for k, c in width.items():
            t = item[k]
            assert t.shape == (156, c), (k, t.shape)
            assert torch.equal(t[:rows], labels[("key_labels", "key_signature_id", "genre", "tonic_labels").index(k)].expand(rows, c))
            assert not t[rows:].any()                                          # zero padding behind the clip's rows
        assert item["mel"].shape == (1, 288, 156) and not item["mel"][..., T:].any()
        if genre:
            assert float(item["genre"][0].sum()) == (0.0 if i == 1 else 1.0)  # one-hot (11), all-zero row for a clip without a genre
        else:
            assert not item["genre"].any()                                    # zeros(8)


def test_batches_collate_with_seq_length():
    ds, _ = build(False, [61, 101, 156], ["A minor", "C major", "F# minor"])
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False)))
    assert batch["mel"].shape == (3, 1, 288, 156)
    assert batch["key_labels"].shape == (3, 156, 12) and batch["key_signature_id"].shape == (3, 156, 24)
    assert batch["seq_length"].tolist() == [61, 101, 156]
    valid = batch["seq_length"] - SPAN + 1                                     # the rows general_step scores per clip
    for i, n in enumerate(valid.tolist()):
        assert batch["tonic_labels"][i, :n].sum(1).eq(1).all() and not batch["tonic_labels"][i, n:].any()


def test_local_labels_helper():
    labels = (torch.arange(12.0), torch.arange(24.0), torch.zeros(8), torch.ones(12))
    out = local_labels(labels, 60, local_opt())
    assert [tuple(t.shape) for t in out] == [(11, 12), (11, 24), (11, 8), (11, 12)]
    assert all(torch.equal(o, t.expand_as(o)) for o, t in zip(out, labels))
    assert tuple(local_labels(labels, 30, local_opt(frames=2))[0].shape) == (11, 12)
    assert torch.equal(pad_rows(out[0], 15)[11:], torch.zeros(4, 12))


def test_too_short_clip_is_refused_by_name():
    with pytest.raises(ValueError, match=r"clips/1.*49 CQT frames"):
        build(False, [61, 49, 156], ["A minor", "C major", "F# minor"])
    ds, _ = build(False, [50], ["A minor"])                                   # one window exactly: one labelled row
    assert ds[0]["key_labels"][:1].sum() == 7 and ds[0]["seq_length"] == 50


def test_whole_song_local_is_refused():
    with pytest.raises(ValueError, match="--frames > 0"):
        ake_amd.KeyDataset(False, local_opt(frames=0))
