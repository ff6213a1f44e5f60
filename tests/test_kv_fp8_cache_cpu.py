"""KvFp8Cache (dia_hip/engine.py), the holder of an e4m3 K/V cache's four tensors, on CPU tensors: what it allocates, what it counts
and which addresses it hands to the library."""
import torch

from dia_hip import binding as hb
from dia_hip.engine import KvFp8Cache


def test_shapes_dtypes_bytes_and_pointers():
    c = KvFp8Cache(2, 2, 2, 64)
    assert c.k8.shape == (2, 2, 2, 64, 128) and c.v8.shape == (2, 2, 2, 2, 128, 32) and c.ks.shape == c.vs.shape == (2, 2, 2, 64)
    assert c.k8.dtype == c.v8.dtype == torch.uint8 and c.ks.dtype == c.vs.dtype == torch.float32
    assert all(int(t.count_nonzero()) == 0 for t in (c.k8, c.v8, c.ks, c.vs))
    assert c.nbytes == sum(t.numel() * t.element_size() for t in (c.k8, c.v8, c.ks, c.vs)) == 2 * (2 * 2 * 64) * (128 + 128 + 4 + 4)
    whole, arr = c.ptrs(), c.ptr_array()
    assert isinstance(whole, hb.KvFp8Ptrs) and len(arr) == 2 and isinstance(arr[0], hb.KvFp8Ptrs)
    assert (whole.k8, whole.v8, whole.ks, whole.vs) == (c.k8.data_ptr(), c.v8.data_ptr(), c.ks.data_ptr(), c.vs.data_ptr())
    for i in range(2):
        want = (c.k8[i].data_ptr(), c.v8[i].data_ptr(), c.ks[i].data_ptr(), c.vs[i].data_ptr())
        for p in (c.ptrs(i), arr[i]):
            assert (p.k8, p.v8, p.ks, p.vs) == want
    assert c.ptrs(1).k8 - c.ptrs(0).k8 == 2 * 2 * 64 * 128 and c.ptrs(1).ks - c.ptrs(0).ks == 2 * 2 * 64 * 4
