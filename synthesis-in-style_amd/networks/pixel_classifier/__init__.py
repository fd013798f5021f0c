"""DatasetGAN pixel classifiers (reference: networks/pixel_classifier/model.py)."""
from networks.pixel_classifier.model import PixelClassifier, PixelEnsembleClassifier, ensemble_eval_mode  # noqa: F401
