"""The three helpers of the reference's segmentation/gan_local_edit/ptutils.py:25-95 that the catalogs use."""
import torch


def partial_flat(x):
    """[N, C, H, W] -> [N*H*W, C] (row (n H + h) W + w).  Kept for callers: the device fit reads the 4-D tensor in place."""
    flat = x.permute(0, 2, 3, 1).contiguous().view(-1, x.shape[1])
    flat.original_shape = x.shape
    return flat


def partial_unflat(x, N=None, H=None, W=None):
    assert x.dim() == 2
    C = x.shape[1]
    if N is None:
        N, C, H, W = x.original_shape
    if W is None:
        W = H
    assert N is not None and H is not None and W is not None
    return x.view(N, H, W, C).permute(0, 3, 1, 2)


class MultiResolutionStore:
    """One tensor [..., res, res] and resized copies of it, made on demand ('nearest' or 'bilinear')."""

    def __init__(self, item=None, interpolation_mode='bilinear'):
        self._data = {}
        self._res = None
        if item is not None:
            self._res = item.shape[-1]
            self._data[self._res] = item
        self.interpolation_mode = interpolation_mode

    def get(self, res=None, make=True):
        res = self._res if res is None else res
        if res not in self._data and make:
            self._data[res] = torch.nn.functional.interpolate(self._data[self._res], size=(int(res), int(res)),
                                                              mode=self.interpolation_mode)
        return self._data[res]

    def __getitem__(self, res):
        return self.get(res, make=False)

    def __contains__(self, res):
        return res in self._data

    def __len__(self):
        return len(self._data)

    def resolutions(self):
        return iter(self._data.keys())

    def __repr__(self):
        return 'MultiResolutionStore {}: {}'.format(tuple(self._data[self._res].shape), list(self.resolutions()))
