"""k-means catalogs of generator activations on the MI355X: fitting and nearest-centre assignment.

Mirrors the reference ``FactorCatalog`` (segmentation/gan_local_edit/factor_catalog.py:18-79).

``predict(X[B,C,H,W]) -> int64 [B,H,W]`` = ``argmin_k ||x - centre_k||^2`` per pixel.  The reference moves the activations to
the CPU and builds an N x K x C difference tensor there (6.7 GB for B=10, K=20 at 256^2); here one HIP kernel reads the
activation once on the device and writes the label map (sis_hip.kmeans_assign).

``fit_predict(X, raw=False)`` fits the centres with ``MiniBatchSphericalKMeans`` on the device (spherical_kmeans.py,
csrc/spherical_kmeans.hip) and returns the one-hot heatmaps of its ``labels_``.

A quirk of the reference that is kept, not fixed: ``predict`` measures the Euclidean distance of the UN-normalised pixel to the
unit centres (its ``pairwise_distance``), while the fit labels the unit-normalised pixel.  ``predict(X)`` may therefore differ
from the ``labels_`` that ``fit_predict(X)`` returned for the same ``X``; the dataset loop uses ``predict``, as the reference does.
"""
import torch

import sis_hip
from segmentation.gan_local_edit import ptutils
from segmentation.gan_local_edit.spherical_kmeans import MiniBatchSphericalKMeans


class FactorCatalog:
    def __init__(self, k=None, random_state=0, cluster_centers=None, factorization=None, **kwargs):
        self.k = k
        self.cluster_centers = None if cluster_centers is None else torch.as_tensor(cluster_centers, dtype=torch.float32)
        self.annotations = {}
        self._factorization = None
        if k is not None and cluster_centers is None:
            self._factorization = (factorization or MiniBatchSphericalKMeans)(n_clusters=k, random_state=random_state, **kwargs)

    def pairwise_distance(self, X):
        """X: [N, C] flattened pixels (ptutils.partial_flat layout) -> nearest centre id per row."""
        n, c = X.shape
        return self._assign(X.t().reshape(1, c, n, 1)).reshape(n)

    def _assign(self, X):
        if self.cluster_centers is None:
            raise RuntimeError("FactorCatalog has no cluster centres (fit_predict first, or load a fitted catalog)")
        sis_hip.require_device(X, "X")
        if self.cluster_centers.device != X.device:
            self.cluster_centers = self.cluster_centers.to(X.device)
        return sis_hip.kmeans_assign(X, self.cluster_centers)

    def fit_predict(self, X, raw=False):
        """Fit the catalog on the activation X [B,C,H,W] (device) and return the heatmaps of the fit's own labels:
        ``raw=True``: one-hot [B,k,H,W] in a ``MultiResolutionStore('nearest')``; else the annotation-merged heatmaps and the
        annotation names.  Afterwards ``cluster_centers`` is set and ``predict`` works (see the module docstring for how
        ``predict(X)`` can differ from these labels)."""
        if self._factorization is None:
            raise RuntimeError("FactorCatalog was built from given centres or without k: nothing to fit")
        self._factorization.fit(X)
        self.cluster_centers = torch.from_numpy(self._factorization.cluster_centers_).to(X.device)
        b, _, h, w = X.shape
        k = self.cluster_centers.shape[0]
        labels = self._factorization.labels_.reshape(b, h, w)
        heatmaps = torch.nn.functional.one_hot(labels, k).permute(0, 3, 1, 2).float()
        if raw:
            return ptutils.MultiResolutionStore(heatmaps, 'nearest')
        merged = torch.cat([heatmaps[:, v].sum(1, keepdim=True) for v in self.annotations.values()], 1)
        return ptutils.MultiResolutionStore(merged, 'nearest'), list(self.annotations.keys())

    @property
    def labels_(self):
        return None if self._factorization is None else self._factorization.labels_

    def predict(self, X):
        batch_size, _, height, width = X.shape
        return self._assign(X).reshape(batch_size, height, width)

    def __repr__(self):
        return '{} catalog:\n\t{}'.format(type(self._factorization), self.annotations)
