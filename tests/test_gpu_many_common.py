"""many_common.upload / download on the device: one transfer each way, the values and shapes of the inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_upload_of_a_mixed_list_and_download(pack):
    from egregora_amd.many_common import download, upload
    dev = torch.device("cuda", torch.cuda.current_device())
    a = (torch.arange(6, dtype=torch.float64).view(3, 2) / 7.0).t()                   # host float64 [2, 3], a transposed view
    b = torch.full((1, 1), 0.25, dtype=torch.float32, device=dev)
    assert tuple(a.shape) == (2, 3) and not a.is_contiguous()
    ups = upload([a, b], dev, torch.float32)
    assert all(u.is_cuda and u.is_contiguous() and u.dtype == torch.float32 for u in ups)
    assert torch.equal(ups[0].cpu(), a.to(torch.float32)) and tuple(ups[0].shape) == (2, 3)
    assert ups[1].data_ptr() == b.data_ptr() and torch.equal(ups[1], b)               # already there: taken as it is
    c = torch.arange(6, dtype=torch.int32).view(3, 2) - 2
    (ci,) = upload([c], dev, torch.int32)
    assert ci.is_cuda and ci.is_contiguous() and ci.dtype == torch.int32 and torch.equal(ci.cpu(), c)
    assert upload([], dev, torch.float32) == []
    xs = [torch.full((1, 1), 3.0, device=dev), torch.arange(10, dtype=torch.float32, device=dev).view(2, 5),
          torch.arange(4, dtype=torch.float32, device=dev).view(4, 1) - 1.5]
    ys = download(xs)
    assert [tuple(y.shape) for y in ys] == [(1, 1), (2, 5), (4, 1)]
    assert all(not y.is_cuda and y.dtype == torch.float32 and torch.equal(y, x.cpu()) for x, y in zip(xs, ys))
    assert download([]) == []
