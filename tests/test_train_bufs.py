"""The weight-grad buffer cache of the fused train path is keyed by
id(parameter); a freed model's ids come back for other parameters of the
next model in the same process, so a reused id must not return buffers of
another shape."""

import torch


def test_reused_key_with_other_shapes_gets_its_own_buffers():
    from roko_amd.ops.train import _wgrad_bufs

    dev = torch.device("cpu")
    key = 0x7F00DEADBEEF  # stands for an id() that two parameters shared
    a = _wgrad_bufs(key, dev, (768, 256), (768,))
    assert [tuple(t.shape) for t in a] == [(768, 256), (768,)]
    b = _wgrad_bufs(key, dev, (768, 500), (768,))
    assert [tuple(t.shape) for t in b] == [(768, 500), (768,)]
    c = _wgrad_bufs(key, dev, (5, 256), (5,), (3,))
    assert len(c) == 3
    # the same key and shapes ping-pong over two sets, as before
    a2 = _wgrad_bufs(key, dev, (768, 256), (768,))
    a3 = _wgrad_bufs(key, dev, (768, 256), (768,))
    assert a2[0] is not a[0] and a3[0] is a[0]
