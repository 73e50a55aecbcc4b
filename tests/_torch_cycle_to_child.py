"""Child process of tests/test_gpu_cycle_to.py: the out-of-place entry points on PyTorch memory and streams, and under hipGraph
capture.  torch is imported FIRST so that its bundled HIP runtime is the one libmodgpu.so binds to (one runtime per process)."""
import os
import sys

import torch  # noqa: E402  (must precede modulate_amd's first use)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import modulate_amd as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

assert torch.cuda.is_available() and M.device_count() >= 1

# (1) views as src and dst (t[3:] and u[5:]), on a torch side stream; the source tensor is not mutated
n = 5_000_011
pt = O.splitmix_bytes(n + 8, 77)
t = torch.from_numpy(pt.copy()).cuda()
u = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
src, dst = t[3:3 + n], u[5:5 + n]
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    M.cycle_device_to(dst.data_ptr(), src.data_ptr(), n, M.KEY_PS3, 0, 0, side.cuda_stream)
side.synchronize()
want = pt[3:3 + n].copy()
O.cycle(want, O.KEY_PS3)
assert np.array_equal(dst.cpu().numpy(), want), "torch view / stream mismatch"
assert np.array_equal(t.cpu().numpy(), pt), "the source tensor changed"
assert not u[:5].cpu().numpy().any() and not u[5 + n:].cpu().numpy().any(), "bytes around the destination view changed"
assert M.last_launch()["variant"] == 5

# (2) captured into a CUDAGraph: out of place is idempotent, so EVERY replay gives the same dst, and src never changes
def capture_and_replay(n, ps, pd, key, so, check):
    pt = O.splitmix_bytes(n + 16, 5)
    t = torch.from_numpy(pt).cuda()
    u = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        M.cycle_device_to(u[pd:].data_ptr(), t[ps:].data_ptr(), n, key, so, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not u.cpu().numpy().any(), "capture must record, not execute"
    for k in range(3):
        u.zero_()
        g.replay()
        torch.cuda.synchronize()
        check(u[pd:pd + n], pt[ps:ps + n], k)
        assert not u[:pd].cpu().numpy().any() and not u[pd + n:].cpu().numpy().any()
        assert np.array_equal(t.cpu().numpy(), pt), f"graph replay {k} changed the source"


def whole(key, so):
    def check(d, p, k):
        w = p.copy()
        O.cycle_at(w, key, so)
        assert np.array_equal(d.cpu().numpy(), w), f"graph replay {k}"
    return check


capture_and_replay((3 << 20) + 123, 3, 0, M.KEY_PS4, 0, whole(M.KEY_PS4, 0))
capture_and_replay((1 << 20) + 7, 1, 6, 0x7FFFFFFF, 9, whole(0x7FFFFFFF, 9))  # zero-residue key: a captured copy


# (3) a 320 MiB capture: checked on windows across the buffer
def windows(key, so):
    def check(d, p, k):
        n = p.size
        for off in (0, (100 << 20) + 7, n - (1 << 20)):
            w = p[off:off + (1 << 20)].copy()
            O.cycle_at(w, key, so + off)
            assert np.array_equal(d[off:off + (1 << 20)].cpu().numpy(), w), ("320 MiB replay", k, off)
    return check


capture_and_replay((320 << 20) + 48, 5, 0, M.KEY_PS4, 12345, windows(M.KEY_PS4, 12345))
print("TORCH_CYCLE_TO_OK")
