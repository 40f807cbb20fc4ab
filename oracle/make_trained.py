"""Recipe of tests/golden/pcnet_trained.npz: weights whose outputs depend on the input.

TEST INFRASTRUCTURE ONLY.  Runs on the CPU in about half a minute and needs neither the reference tree nor a GPU:

    python -m oracle.make_trained

36 Adam steps (lr 1e-3, no decay) of the float32 oracle loop (oracle/fit_oracle.py) from tests/golden/pcnet_default.npz: batches of 8,
clips 0..95 of ake_amd.synthetic through cqt_oracle.FastDirectCQT (float64, cast to float32), three epochs in order.  The loss falls from
about 3.2 to about 1.5; on the held-out clips 200..207 the key output spans 0..1 and the tonic several units, where the seeded fixture
gives 0.5251 in every class for any input.

The file holds the float32 state_dict, `opt`, the recipe's parameters, the loss curve, and the float64 oracle's outputs on clips
200..207 with seq_length = [76, 70, 61, 50, 76, 76, 40, 33].  The mel is not stored: tests recompute it (tests/sensitive.py::trained_mel).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
RECIPE = dict(start="pcnet_default.npz", lr=1e-3, batch=8, first_clip=0, clips=96, epochs=3, dtype="float32", seed_note="no random draw: batches in order",
              eval_first_clip=200, eval_seq_length=[76, 70, 61, 50, 76, 76, 40, 33])


def main():
    sys.path.insert(0, REPO)
    from ake_amd import synthetic
    from oracle import cqt_oracle, pcnet_oracle
    from oracle.fit_oracle import oracle_fit

    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    gold = np.load(os.path.join(GOLD, RECIPE["start"]), allow_pickle=False)
    sd32 = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("sd/")}
    cq = cqt_oracle.FastDirectCQT(synthetic.SR, cqt_oracle.hop_for(synthetic.SR), dtype=torch.float64)

    def mel_of(indices):
        ys, labels = synthetic.make_batch(indices)
        return torch.as_tensor(cq(ys))[:, None], labels

    B = RECIPE["batch"]
    batches = []
    for lo in range(RECIPE["first_clip"], RECIPE["first_clip"] + RECIPE["clips"], B):
        mel, lb = mel_of(range(lo, lo + B))
        batches.append({"mel": mel.float(), "seq_length": torch.full((B,), mel.shape[3]), "key_labels": torch.from_numpy(lb["key_labels"]),
                        "tonic_labels": torch.from_numpy(lb["tonic_labels"]), "genre": torch.from_numpy(lb["genre"]),
                        "key_signature_id": torch.from_numpy(lb["key_signature_id"])})
    batches = batches * RECIPE["epochs"]
    losses, sd = oracle_fit(sd32, None, batches, 1, len(batches), lr=RECIPE["lr"], dtype=torch.float32)
    print(f"{len(losses)} steps: loss {np.mean(losses[:4]):.3f} -> {np.mean(losses[-4:]):.3f}")
    sd = {k: v.detach().clone() for k, v in sd.items()}

    seq = torch.tensor(RECIPE["eval_seq_length"])
    x, _ = mel_of(range(RECIPE["eval_first_clip"], RECIPE["eval_first_clip"] + len(seq)))
    with torch.no_grad():
        key, tonic, genre = pcnet_oracle.pcnet_forward(pcnet_oracle.to_dtype(sd, torch.float64), x, seq)
    print("held-out clips: key %.3f .. %.3f, tonic %.2f .. %.2f" % (float(key.min()), float(key.max()), float(tonic.min()), float(tonic.max())))
    path = os.path.join(GOLD, "pcnet_trained.npz")
    np.savez_compressed(path, opt=str(gold["opt"]), recipe=json.dumps(RECIPE), losses=np.asarray(losses, np.float64), seq_length=seq.numpy(),
                        key=key.numpy(), tonic=tonic.numpy(), genre=genre.numpy(),
                        **{"sd/" + k: (v.numpy().astype(np.float32) if v.is_floating_point() else v.numpy()) for k, v in sd.items()})
    prov_path = os.path.join(GOLD, "PROVENANCE.json")
    with open(prov_path) as f:
        prov = json.load(f)
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    prov["pcnet_trained.npz"] = {"recipe": "python -m oracle.make_trained (CPU only, no reference tree)", "parameters": RECIPE, "torch": torch.__version__,
                                 "loss_first4_last4": [float(np.mean(losses[:4])), float(np.mean(losses[-4:]))], "sha256": digest,
                                 "bytes": os.path.getsize(path)}
    with open(prov_path, "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
