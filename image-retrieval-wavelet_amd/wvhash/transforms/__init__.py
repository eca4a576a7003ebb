from .custom_transforms import (SWTTransform, DWTTransform, RawStackTransform, BaseWaveletTransform,
                                find_wavelet_transform)
from .functional import (swt2d, swt2d_band, swt2d_band_host, dwt2d, rawstack, swt2d_host, dwt2d_host, rawstack_host, swt2d_place_output, size_images, size_images_host,
                         lift_images, lift_images_host)
from .wavelets import get_filters, wavelist
from .pil_ops import (Resize, CenterCrop, RandomResizedCrop, RandomCrop, RandomHorizontalFlip, ColorJitter, ToTensor, Normalize, Compose,
                      build_transform)
from .sizing import RawBatch, RawItem, LazyImage, raw_collate
from .lifting import CustomTransform, ResizeSubBands, HaarLifting, Cdf97Lifting, TensorTailTransform

__all__ = ["SWTTransform", "DWTTransform", "RawStackTransform", "BaseWaveletTransform", "find_wavelet_transform", "swt2d", "swt2d_band", "swt2d_band_host", "swt2d_place_output", "swt2d_host", "dwt2d_host", "rawstack_host",
           "dwt2d", "rawstack", "get_filters", "wavelist", "Resize", "CenterCrop", "Compose", "build_transform", "CustomTransform", "ResizeSubBands", "HaarLifting",
           "Cdf97Lifting", "size_images", "size_images_host", "RandomResizedCrop", "RandomHorizontalFlip", "ColorJitter", "RawBatch", "RawItem", "LazyImage", "raw_collate",
           "lift_images", "lift_images_host", "RandomCrop", "ToTensor", "Normalize", "TensorTailTransform"]
