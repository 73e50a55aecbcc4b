"""Child process of tests/test_gpu_xfer.py: the transfer entry points with PyTorch tensors as the device side.  torch is imported FIRST
so that its bundled HIP runtime is the one libmodgpu.so binds to (one runtime per process)."""
import os
import sys

import torch  # noqa: E402  (must precede modulate_amd's first use)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import modulate_amd as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

assert torch.cuda.is_available() and M.device_count() >= 1

# (1) a tensor view as the upload's destination: the bytes around the view stay as they were
n = 5_000_011
pt = O.splitmix_bytes(n, 78)
u = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()  # (the call does not order itself against torch's streams)
M.cycle_host_to_device(u[5:].data_ptr(), pt, M.KEY_PS3, 0, 0)
want = pt.copy()
O.cycle(want, O.KEY_PS3)
got = u.cpu().numpy()
assert np.array_equal(got[5:5 + n], want), "upload into a tensor view"
assert not got[:5].any() and not got[5 + n:].any(), "bytes around the destination view changed"

# (2) a tensor as the download's source: the tensor is not changed, the thread's current device is kept
t = torch.from_numpy(want.copy()).cuda()
torch.cuda.synchronize()
out = np.zeros(n, np.uint8)
M.cycle_device_to_host(out, t.data_ptr(), M.KEY_PS3, 0, -1)
assert np.array_equal(out, pt), "download from a tensor"
assert np.array_equal(t.cpu().numpy(), want), "the source tensor changed"
assert torch.cuda.current_device() == 0

# (3) a CPU tensor's pointer is not device memory: refused before anything is queued
c = torch.zeros(4096, dtype=torch.uint8)
try:
    M.cycle_host_to_device(c.data_ptr(), pt[:100], 1)
    raise SystemExit("a host pointer was accepted as the device side")
except M.ModGpuError as e:
    assert e.code == 1, e
print("TORCH_XFER_OK")
