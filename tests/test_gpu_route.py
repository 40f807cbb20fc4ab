"""GPU: what the forward pass's route promises is what the forward does.

The route is decided once per call; ``ake_pcnet_accepts_frames_major`` and the debug taps answer from the same
decision.  These tests hold the answers against the behaviour: the frames-major flag against the frames-major forward, the two
kinds of remainder chunk against forwards of their own, and the taps against the float64 oracle's activations.
"""
import pytest
import torch

import ake_amd
from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle
from test_gpu_pcnet import TOL, _check_taps
from test_gpu_pipeline import default_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def net(gold_default):
    n = ake_amd.PitchClassNet(288, 12, 2, 7, default_opt())
    n.load_state_dict(golden_state_dict(gold_default), strict=True)
    return n.to(DEV).eval()


def _mel(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, 1, 288, T), generator=g) * 2.5).to(DEV)


@pytest.mark.parametrize("T", [40, 74, 76, 77])
def test_frames_major_answer_equals_the_behaviour(net, T):
    """ake_pcnet_accepts_frames_major is 1 exactly where ake_pcnet_forward_frames_major_f32 runs, and there the three outputs equal
    ake_pcnet_forward_f32 on the transposed input bit for bit; elsewhere the call is refused by name before any launch.  (Where the
    answer turns between batch sizes depends on the CU count -- the persistent first pitch conv wants two row tiles per CU -- so
    the crossing point is not asserted, only that both answers occur at 76 frames.)"""
    L = ake_amd._lib.lib()
    batches = (1, 2, 16, 17, 18, 19, 24)
    x = _mel(max(batches), T, 300 + T)
    x_fm = x[:, 0].transpose(1, 2).contiguous()                       # [clip][frame][bin]
    stream = torch.cuda.current_stream().cuda_stream
    answers = []
    for B in batches:
        seq = torch.full((B,), T, dtype=torch.int64, device=DEV)
        want = net(x[:B], seq)                                        # (also creates the handle)
        acc = L.ake_pcnet_accepts_frames_major(net.handle, B, T)
        assert acc in (0, 1), (B, T, acc)
        answers.append(acc)
        outs = [torch.full((B, n), -7.0, dtype=torch.float32, device=DEV) for n in (12, 12, 11)]
        ws = torch.empty(L.ake_pcnet_workspace_bytes(net.handle, B, T), dtype=torch.uint8, device=DEV)
        ake_amd._lib.prof_enable("", True)
        try:
            rc = L.ake_pcnet_forward_frames_major_f32(net.handle, x_fm.data_ptr(), B, T, seq.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                      outs[2].data_ptr(), ws.data_ptr(), ws.numel(), stream)
            err = L.ake_last_error()
            launched = ake_amd._lib.prof_results()
        finally:
            ake_amd._lib.prof_enable("", False)
        assert (rc == 0) == (acc == 1), (B, T, rc, acc)
        if acc:
            for a, b in zip(outs, want):
                assert torch.equal(a, b), (B, T)
        else:
            assert b"frames-major" in err, (B, T, err)
            assert not launched, (B, T, sorted(launched))
            assert all(bool((o == -7.0).all()) for o in outs), (B, T)
    if T == 76:
        assert 0 in answers and 1 in answers, answers                # the sweep must see both routes
    if T == 77:
        assert not any(answers), answers                              # an odd frame count never takes the persistent pitch conv


@pytest.fixture(scope="module")
def chunk_case(net):
    """288 clips x 76 frames and the forward of the first 256 on their own (one full pitch-stream chunk)."""
    x = _mel(288, 76, 41)
    g = torch.Generator().manual_seed(42)
    seq = torch.randint(40, 77, (288,), generator=g).to(DEV)
    full = [t.clone() for t in net(x[:256], seq[:256])]
    return x, seq, full


@pytest.mark.parametrize("rem", [1, 32])
def test_remainder_chunk(net, chunk_case, rem):
    """256 + 1 and 256 + 32 clips.  A one-clip remainder cannot take the persistent first pitch conv, so the whole call falls back
    from the f16 up_sixth map (layer 0 writes it for every clip before any chunk runs); a 32-clip remainder can take it.  Either
    way every clip equals its result in a call without a remainder."""
    x, seq, full = chunk_case
    B = 256 + rem
    outs = net(x[:B], seq[:B])
    own = net(x[256:B], seq[256:B])
    for name, a, f, o in zip(("key", "tonic", "genre"), outs, full, own):
        e_full, e_own = rel_err(a[:256], f), rel_err(a[256:], o)
        print(f"remainder {rem} {name}: rows [0, 256) vs the 256-clip call {e_full:.2e}, rows [256, {B}) vs their own call {e_own:.2e}")
        assert e_full < TOL and e_own < TOL, (name, e_full, e_own)


def _held_or_served(net, name, B, T, ref):
    """`name` is the up_sixth map layer 0 hands to the first pitch conv: f16 x 4 words exactly where that conv is the persistent
    kernel for the whole call -- which, for this net, is where the call could also read mel frames-major -- and f32 elsewhere."""
    if ake_amd._lib.lib().ake_pcnet_accepts_frames_major(net.handle, B, T):
        with pytest.raises(ake_amd._lib.AkeError, match="held as f16 words"):
            net.tap(name)
        return True
    got = net.tap(name).cpu().numpy()
    assert got.shape == ref.shape and rel_err(got, ref) < 1e-3, (name, B, T, rel_err(got, ref))
    return False


def test_taps_are_exact(net, gold_default):
    """The taps answer from the route of the forward that ran: refused exactly where that forward kept the activation out of memory,
    served (and right) where it wrote it.

    4 x 76 without keep_taps: layer 0's stack stays in LDS, the last pitch conv is fused with the semitone conv, the last
    pitch-class stack is one launch -- four refusals with the texts they always had.  `model.1.up_sixth_a` is the fifth name the
    tap used to refuse at this shape ("may be held as f16 words"): the forward holds it as f16 words only when the persistent
    kernel reads it, which needs two row tiles per CU -- 4 clips x 29 tiles are too few on any part with more than 58 CUs, the map
    is then written as f32 and the exact tap serves it.  So that name is held to the stronger of the two: refused where it is
    held as words, else equal to the oracle's activation; both outcomes must occur (4 and 64 clips).
    2 x 100: neither one-launch form of layer 0 fits the LDS; the per-stage kernels write the stack and the map as f32.
    4 x 76 with keep_taps: every name _check_taps lists, in its layout (NCHW / split planes / one f16 plane), through its values."""
    sd64 = golden_state_dict(gold_default, torch.float64)
    was = net.keep_taps(False)
    try:
        x = _mel(4, 76, 7)
        seq = torch.full((4,), 76, dtype=torch.int64, device=DEV)
        taps76 = {}
        ref76 = pcnet_oracle.pcnet_forward(sd64, x.cpu().double(), seq.cpu(), taps=taps76)
        net(x, seq)
        for name, text in (("model.0.pc2pc.layer.2", "stays in LDS"), ("model.0.pc2pc.layer.5", "stays in LDS"),
                           ("model.1.p2p.layer.8", "fused with the semitone conv"), ("model.1.pc2pc.layer.5", "stays in LDS")):
            with pytest.raises(ake_amd._lib.AkeError, match=text):
                net.tap(name)
        held = [_held_or_served(net, "model.1.up_sixth_a", 4, 76, taps76["model.1.up_sixth_a"].numpy())]
        xb = torch.cat([x] * 16)
        net(xb, torch.full((64,), 76, dtype=torch.int64, device=DEV))
        held.append(_held_or_served(net, "model.1.up_sixth_a", 64, 76, torch.cat([taps76["model.1.up_sixth_a"]] * 16).numpy()))
        assert True in held and False in held, held
        x2 = _mel(2, 100, 9)
        seq2 = torch.full((2,), 100, dtype=torch.int64, device=DEV)
        net(x2, seq2)
        taps = {}
        pcnet_oracle.pcnet_forward(sd64, x2.cpu().double(), seq2.cpu(), taps=taps)
        for name in ("model.0.pc2pc.layer.2", "model.0.pc2pc.layer.5", "model.1.up_sixth_a"):
            got = net.tap(name).cpu().numpy()
            ref = taps[name].numpy()
            assert got.shape == ref.shape, name
            err = rel_err(got, ref)
            print(f"tap {name} at 2 x 100: {err:.2e}")
            assert err < 1e-3, (name, err)                            # (the bound _check_taps gives these three names)
        net.keep_taps(True)
        outs = net(x, seq)
        gold = {"tap/" + k: v.numpy() for k, v in taps76.items()}
        gold.update({n: r.numpy() for n, r in zip(("key", "tonic", "genre"), ref76)})
        _check_taps(net, outs, gold)
    finally:
        net.keep_taps(was)
