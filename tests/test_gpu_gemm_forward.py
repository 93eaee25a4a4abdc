"""``-m gpu``: the forward GEMMs of csrc/gemm.hip, one launch each through ``mra_debug_gemm`` (launch_gemm behind host checks), for every case of
the table in ``tests/gemm_cases.py`` -- the launch forms of the Q-Former layer chain, the folded cross-attention, the K/V projection and
mra_llm_proj -- in f16 and bf16, against float64 references on the same rounded inputs under the DERIVED bounds of that file (nothing there
was fitted to this file's output; tests/test_gemm_cases_cpu.py holds the fp32 emulations inside every bound, the named mutants outside, and
the table to the kernel families it names).  Every test asserts the family that ran (the launch counters) and max |d| / bound <= 1, and prints
the ratio.

Canaries as tests/test_gpu_qformer_kernels.py: every output buffer is all-ones bits between guards; after the launch exactly the owned elements
were rewritten (the overhang columns of an n_ragged fp32 launch may be), the guards are intact; inputs hold NaN wherever no view addresses
them and come back bit for bit.  An EPI_RES_LN case is launched twice in a row on the same counters, which nothing clears in between."""
import time

import pytest
import torch

import gemm_cases as G
from mraudio_amd import _lib as L
from test_gpu_qformer_kernels import DEV, GUARD, Buf, _bits, _ok, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


def _after(buf, what):
    """The inside of an output buffer on the CPU, after checking its guards."""
    bits = _bits(buf.buf).cpu()
    for sl in (slice(0, GUARD), slice(GUARD + buf.numel, None)):
        assert torch.equal(bits[sl], buf.before[sl]), f"{what}: a guard was written"
    return buf.inner.cpu()


def _launch(c, dt, ins, counters):
    """One mra_debug_gemm call over the case's problems: fresh output buffers, the given counter buffer.  Returns the outputs on the CPU."""
    dtype = G.DTYPES[dt]
    outs = [{k: Buf(v.numel(), v.dtype) for k, v in o.items()} for o in G.fresh_outputs(c, dt)]

    def addr(i, b):
        if b == "ln_counter":
            buf = counters
        else:
            buf = ins[i].get(b) or outs[i].get(b)
        if buf is None:
            return None
        return buf.inner.data_ptr(), buf.numel * buf.inner.element_size()

    arr = G.descriptors(c, dt, addr)
    fams = range(L.GEMM_FAMILIES)
    before = [L.gemm_launches(f, c["epi"]) for f in fams]
    _ok(L.lib().mra_debug_gemm(arr, len(c["probs"]), c["epi"], L.mra_dtype(dtype), _stream()), f"mra_debug_gemm {c['name']}")
    ran = [L.gemm_launches(f, c["epi"]) - b for f, b in zip(fams, before)]
    assert ran == [int(f == c["family"]) for f in fams], f"families launched {ran}, expected family {c['family']}"
    for i, d in enumerate(ins):
        for k, buf in d.items():
            buf.unchanged(f"problem {i} {k}")
    return [{k: _after(buf, f"problem {i} {k}") for k, buf in o.items()} for i, o in enumerate(outs)]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", [c["name"] for c in G.CASES])
def test_forward_gemm_against_float64(name, dt):
    t0 = time.time()
    c = G.BY_NAME[name]
    ins = [{k: Buf(v.numel(), v.dtype, v) for k, v in d["flat"].items()} for d in G.inputs(name, dt)]
    counters = None
    if c["epi"] == G.EPI_RES_LN:
        counters = Buf(G.counter_offsets(c)[1], torch.int32, torch.zeros(G.counter_offsets(c)[1], dtype=torch.int32))
    worst, failures = {}, []
    for launch in range(2 if counters else 1):
        outs = _launch(c, dt, ins, counters)
        ratios, fails = G.check(name, dt, outs, _after(counters, "counters") if counters else None)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        failures += [f"launch {launch}: {f}" for f in fails]
    print(f"row {c['row']} {name} {dt} (family {c['family']}): |d| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          f"  [{time.time() - t0:.1f} s]")
    assert not failures, failures[:8]
    assert all(v <= 1.0 for v in worst.values()), worst
