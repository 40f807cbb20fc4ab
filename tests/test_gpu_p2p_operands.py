"""PARITY (GPU): the pitch convs' multiply loop as a software pipeline (A fragments requested three MFMAs ahead into rotating register
slots, the phase's scalars held in registers, the tile sequence walked instead of divided, the semitone conv's B fragments in LDS).

Nothing about the products changed, so the one launch (p2p_stack_kernel, 16 waves) is held torch.equal to the routes that launch each
conv on its own (conv_p2p_f16_ps_kernel: the same loop on 8 waves, other tile heights; conv_p2p_f16_kernel: one workgroup per tile, a
loop of its own) in `model.1.cat`, key, tonic and genre, and three clips of every shape to the float64 oracle at test_gpu_p2p_stack's
tolerance.  Which route a forward took is read from the kernel timer, as there: 1 launch booked as "conv_p2p_f16_kernel" or 3.

The shapes are chosen for what a pipelined loop can get wrong (a request past the patch, a slot read one fragment early or late, a
walked tile base that drifts), not for size.  Tile geometry from p2p_ps_rows' arithmetic for 288 rows and 16 waves, 768 M positions
(row, frame pair) per tile; the folding conv's tile height also divides the octave's 36 rows:

    T   J   rows per tile       tiles  last tile   M positions used   folding conv
    26  13  min(768 / 13) = 59    5    52 rows     767 of 768         36 rows x 8
    30  15  51                    6    33 rows     765                36 rows x 8
    52  26  29                   10    27 rows     754                18 rows x 16
    76  38  20                   15     8 rows     760                18 rows x 16

(26 stands in for the 16 frames first meant here, J = 8: the heads' 12 x 7 convs refuse clips of fewer than 26 frames, so no forward of
this net returns at 16.)  With 8 waves the same shapes give 29 / 25 / 14 / 10 rows per tile (10, 12, 21 and 29 tiles, the last of 27,
13, 8 and 8 rows).  Every shape runs at the smallest batch the one-launch route's gate takes, N - N/16 clips for N CUs; 30 frames also
one clip above the CU count and one below the gate, where the three 8-wave launches run the new loop on whole batches.
"""
import pytest
import torch

from conftest import golden_state_dict, rel_err
from oracle import pcnet_oracle
from test_gpu_p2p_stack import TOL, assert_rows_equal, check_against_separate_launches, forward_timed, inputs, make_net, n_cus

pytestmark = pytest.mark.gpu
SHAPES = [26, 30, 52, 76]


def gate_batch():
    N = n_cus()
    return N - N // 16


@pytest.fixture(scope="module")
def net(gold_default):
    return make_net(gold_default)


@pytest.fixture(scope="module")
def one_launch(net):
    """T -> (x, seq, outputs) of the one-launch route at the gate's smallest batch, each computed once."""
    done = {}

    def get(T):
        if T not in done:
            x, seq = inputs(gate_batch(), T)
            whole, launches = forward_timed(net, x, seq)
            print(f"  T={T} B={x.shape[0]}: {launches} launch(es)")
            assert launches == 1, (T, launches)
            done[T] = (x, seq, whole)
        return done[T]
    return get


@pytest.mark.parametrize("T", SHAPES)
def test_one_launch_equals_separate_launches(net, one_launch, T):
    x, seq, whole = one_launch(T)
    check_against_separate_launches(net, x, seq, whole)


@pytest.mark.parametrize("T", SHAPES)
def test_three_clips_against_the_float64_oracle(gold_default, one_launch, T):
    x, seq, whole = one_launch(T)
    idx = [0, x.shape[0] // 2, x.shape[0] - 1]
    ref = pcnet_oracle.pcnet_forward(golden_state_dict(gold_default, torch.float64), x[idx].cpu().double(), seq[idx].cpu())
    for name, a, b in zip(("key", "tonic", "genre"), whole[:3], ref):
        e = rel_err(a[idx].cpu(), b)
        print(f"  {name}: {e:.2e}", end="")
        assert e < TOL, (name, e)


@pytest.mark.parametrize("extra", [-1, "above"])
def test_eight_wave_launches_on_whole_batches_at_30_frames(net, one_launch, extra):
    """One clip below the gate: three launches on the whole batch.  One clip above the CU count: three launches, or six where the
    pitch stream's chunk splits the batch.  Every clip the one-launch batch also holds equals its result there, and the whole batch
    equals itself as halves and as groups of four."""
    x, seq, whole = one_launch(30)
    B = x.shape[0] - 1 if extra == -1 else n_cus() + 1
    xb, seqb = inputs(B, 30)
    shared = min(B, x.shape[0])
    xb[:shared], seqb[:shared] = x[:shared], seq[:shared]
    tap = B <= n_cus()                                                # (a batch beyond the pitch stream's chunk has no tap)
    got, launches = forward_timed(net, xb, seqb, tap=tap)
    print(f"  T=30 B={B}: {launches} launch(es)")
    assert launches in ((3,) if extra == -1 else (3, 6)), launches
    assert_rows_equal([t[:shared] for t in got], whole[:len(got)], slice(0, shared), f"B = {B}")
    if tap:
        check_against_separate_launches(net, xb, seqb, got)
    else:
        for lo in (0, B - 4):                                         # (four clips: the per-tile kernel, with its tap)
            part, n = forward_timed(net, xb[lo:lo + 4], seqb[lo:lo + 4])
            assert n == 3, n
            assert_rows_equal(part[:3], got, slice(lo, lo + 4), f"clips {lo}:{lo + 4}")
