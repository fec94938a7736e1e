"""The augmentation layer on the native path.

* :mod:`.functional` - the parameter-driven entry functions (parameter dictionaries in, one or two launches out);
* :mod:`.draws` - the host buffer of a call's random draws and its device views;
* :mod:`.base`, :mod:`.modules`, :mod:`.crop_flip` - the modules with the sampling inside the call, in three families (intensity, matrix chain,
  crop / flip);
* :mod:`.container` - ``AugmentationSequential``.
"""
from .container import AugmentationSequential, ParamItem
from .crop_flip import RandomHorizontalFlip, RandomResizedCrop, RandomVerticalFlip
from .functional import (affine_chain, affine_matrix, apply_sequence, color_jitter, gaussian_taps, inverse_chain, perspective_chain, random_affine,
                         random_gaussian_blur, random_perspective, select_samples, warp_pair)
from .modules import ColorJitter, RandomAffine, RandomGaussianBlur, RandomMedianBlur, RandomPerspective

__all__ = ["AugmentationSequential", "ColorJitter", "ParamItem", "RandomAffine", "RandomGaussianBlur", "RandomHorizontalFlip", "RandomMedianBlur", "RandomPerspective",
           "RandomResizedCrop", "RandomVerticalFlip", "affine_chain", "affine_matrix",
           "apply_sequence", "color_jitter", "gaussian_taps", "inverse_chain", "perspective_chain", "random_affine", "random_gaussian_blur",
           "random_perspective", "select_samples", "warp_pair"]
