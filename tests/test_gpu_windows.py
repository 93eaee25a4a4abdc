"""``window_proposal_kernel`` on the GPU against the brute-force host reference of ``tests/window_cases.py``: windows, the fp32 bit
patterns of the scores and the counts must be EQUAL (the definition is in integers: there is no tolerance).  Every launch holds several
videos of different content; the lengths cross the wave (64) and the 512-thread stride boundaries."""
import numpy as np
import pytest
import torch

import window_cases as W
from mraudio_amd import scorer

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 127, 257, 511, 512, 513]
# (top_k, nms_thd, max_len, alpha): every value of every parameter, and every pair of (top_k, nms_thd) and (top_k, max_len)
COMBOS = [(1, 0.0, 0, 0.5), (5, 0.25, 0, 0.5), (64, 0.9, 0, 0.0), (5, 0.0, 1, 0.0), (64, 0.25, 7, 0.5), (1, 0.9, 7, 0.0),
          (64, 0.0, 0, 0.5), (1, 0.25, 1, 0.5), (5, 0.9, 7, 0.5), (64, 0.9, 1, 0.5), (5, 0.25, 7, 0.0), (1, 0.0, 7, 0.5),
          (64, 0.0, 7, 0.0)]


def run_and_compare(x: np.ndarray, alpha, top_k, nms_thd, max_len):
    videos, clips = x.shape
    win, sc, cnt = scorer.windows_from_logits(torch.from_numpy(x).cuda().reshape(-1), videos, clips, alpha, top_k, nms_thd, max_len)
    torch.cuda.synchronize()
    rwin, rsc, rcnt = W.windows_ref(x, videos, clips, alpha, top_k, nms_thd, max_len)
    what = f"V {videos} T {clips} alpha {alpha} top_k {top_k} nms_thd {nms_thd} max_len {max_len}"
    assert win.dtype == torch.int32 and sc.dtype == torch.float32 and cnt.dtype == torch.int32
    assert win.shape == (videos, top_k, 2) and sc.shape == (videos, top_k) and cnt.shape == (videos,)
    assert cnt.cpu().numpy().tolist() == rcnt.tolist(), what
    assert np.array_equal(win.cpu().numpy(), rwin), what
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), rsc.view(np.uint32)), what


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("T", LENGTHS)
def test_kernel_equals_host_reference(family, T):
    k = W.FAMILIES.index(family) * len(LENGTHS) + LENGTHS.index(T)
    x = W.make_batch(family, T, 4, seed=1)
    for j in range(2):    # two parameter sets per (family, length); over the grid every combination is used about 12 times
        top_k, nms_thd, max_len, alpha = COMBOS[(2 * k + j) % len(COMBOS)]
        run_and_compare(x, alpha, top_k, nms_thd, max_len)


def test_every_parameter_value_on_one_input():
    x = W.make_batch("quant", 65, 4, seed=2)
    for top_k, nms_thd, max_len, alpha in COMBOS:
        run_and_compare(x, alpha, top_k, nms_thd, max_len)


def test_t1024_unlimited():
    """524 800 windows per video, two starts per thread."""
    run_and_compare(W.make_batch("two_peak", 1024, 2, seed=3), 0.5, 10, 0.25, 0)


def test_t4096_with_a_length_cap():
    """The prefix sums fill LDS to its limit; eight starts per thread."""
    run_and_compare(W.make_batch("normal", 4096, 2, seed=4), 0.5, 10, 0.25, 64)


def test_hand_cases_on_the_gpu():
    x = np.asarray([[0, 1, 1, 0, 0, .75, .75, 0]], dtype=np.float32)
    win, sc, cnt = scorer.windows_from_logits(torch.from_numpy(x).cuda().reshape(-1), 1, 8, 0.5, 5, 0.5, 0)
    assert cnt.tolist() == [5] and win[0].tolist() == [[1, 2], [1, 1], [2, 2], [5, 6], [1, 6]] and sc[0].tolist() == [1.0, .5, .5, .5, .5]
    with pytest.raises(scorer.MraError):
        scorer.windows_from_logits(torch.zeros(8, device="cuda"), 1, 8, 0.5, 65)


def test_through_the_model():
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset, collate_fn

    dev = torch.device("cuda:0")
    ds = SyntheticMRDataset(4, T=20, seed=3, duration=40, signal=2.0)
    batch = collate_fn([ds[i] for i in range(4)])
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    model = XInstructBLIP(seed=0, device=dev, top_k=5)
    out = model.encode_fuse(batch)
    torch.cuda.synchronize()
    fused = out["fused"].cpu().numpy()
    rwin, rsc, rcnt = W.windows_ref(fused, 4, 20, 0.5, 5, 0.25, 0)
    assert np.array_equal(out["windows"].cpu().numpy(), rwin)
    assert np.array_equal(out["window_scores"].cpu().numpy().view(np.uint32), rsc.view(np.uint32))
    assert out["window_counts"].cpu().numpy().tolist() == rcnt.tolist()

    texts, records, saliency = model.generate_windows(batch)
    ts = batch["timestamps"]
    for v in range(4):
        want = [[ts[v][s], ts[v][e], float(rsc[v, k])] for k, (s, e) in enumerate(rwin[v, :rcnt[v]].tolist())]
        assert records[v] == want
        assert texts[v] == "[" + ", ".join(f"[{a}, {b}]" for a, b, _ in want) + "]"
        assert np.array_equal(np.asarray(saliency[v], dtype=np.float32), fused.reshape(4, 20)[v])

    plain = XInstructBLIP(seed=0, device=dev)       # the default: today's keys, today's spans
    base = plain.encode_fuse(batch)
    assert not any(k.startswith("window") for k in base)
    assert set(out) - set(base) == {"windows", "window_scores", "window_counts"}
    assert torch.equal(base["spans"], out["spans"])
    with pytest.raises(scorer.MraError):
        plain.generate_windows(batch)
