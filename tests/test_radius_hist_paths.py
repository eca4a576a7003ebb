"""Two paths of the Hamming-radius metrics that tests/test_host_radius_hist.py and tests/test_gpu_radius_hist.py leave out:
class-id labels (1-D, or one column) through CustomCalculator, and the device branch of parallel.sharded_hamming_radius_hist
(PreparedDB / PreparedLabels shards), run shard by shard on one GPU: what each rank computes before the SUM all_reduce."""
import pytest
import torch

import radius_cases as rc
from wvhash import parallel
from wvhash.engine import CustomCalculator
from wvhash.engine import hamming as H
from wvhash.engine import radius_metrics as RM


@pytest.mark.parametrize("column", [False, True])
def test_calculator_takes_class_id_labels(column):
    """Class ids are one-hot onto bits: the numbers are those of the multi-hot form of the same labels."""
    q, r, _, _ = rc.make_inputs(9, 300, 32, 5, seed=4)
    g = torch.Generator().manual_seed(5)
    qid, rid = torch.randint(0, 7, (9,), generator=g), torch.randint(0, 7, (300,), generator=g)
    rid[:8] = qid[:8]
    qid[8] = 9                                                                     # a lone query: no row of its class
    ql, rl = torch.nn.functional.one_hot(qid, 10).float(), torch.nn.functional.one_hot(rid, 10).float()
    want_p = RM.get_precision_recall_by_Hamming_Radius(r, rl, q, ql, radius=3, device="cpu")
    want_P, want_R = RM.pr_curve(q, r, ql, rl, device="cpu")
    assert 0.0 < want_p < 1.0
    calc = CustomCalculator(include=("precision_hamming_radius", "pr_curve_hamming"), device="cpu", hamming_radius=3)
    out = calc.get_accuracy(q, qid[:, None] if column else qid, r, rid[:, None] if column else rid, False)
    assert out["precision_hamming_radius"] == want_p
    assert torch.equal(calc.last_pr_curve_hamming[0], want_P) and torch.equal(calc.last_pr_curve_hamming[1], want_R)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nbits,classes,world", [(1001, 64, 12, 3), (700, 128, 80, 3), (4, 64, 12, 3)])
def test_device_shards_add_up_to_the_unsharded_tables(N, nbits, classes, world):
    """Ragged shards, and (4 rows on 3 ranks) an empty one: a PreparedDB of no rows contributes zeros."""
    q, r, ql, rl = rc.make_inputs(8, N, nbits, classes, seed=N + nbits)
    qp, rp = H.pack_codes(q.cuda()), H.pack_codes(r.cuda())
    qlp, rlp = H.pack_labels(ql.cuda()), H.pack_labels(rl.cuda())
    total = torch.zeros((2, 8, nbits + 2), dtype=torch.int32, device="cuda")
    sizes = []
    for rank in range(world):
        lo, hi, _ = parallel.shard_bounds(N, world, rank)
        sizes.append(hi - lo)
        cum, cumrel = parallel.sharded_hamming_radius_hist(qp, qlp, H.PreparedDB(rp[lo:hi].contiguous(), nbits),
                                                           H.PreparedLabels(rlp[lo:hi].contiguous()), nbits)
        assert cum.is_cuda and cum.dtype == torch.int32 and bool((cum[:, -1] == hi - lo).all())
        total[0] += cum
        total[1] += cumrel
    assert len(set(sizes)) > 1 and (N != 4 or sizes[-1] == 0)
    want = rc.brute_tables(q.cuda(), r.cuda(), ql.cuda(), rl.cuda())
    assert torch.equal(total[0], want[0]) and torch.equal(total[1], want[1])
