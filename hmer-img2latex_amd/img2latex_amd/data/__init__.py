from .augment import Augment, white_fill
from .dataset import (DeviceDataset, DeviceLoader, FormulaStore, PageStore, create_data_loaders, decode_pages_device,
                      loader_settings, read_split)
from .png import PngInfo, parse_png
from .preprocess import batch_convert_for_resnet, load_image, preprocess_batch, preprocess_resident, resize_bilinear

__all__ = ["load_image", "preprocess_batch", "preprocess_resident", "batch_convert_for_resnet", "resize_bilinear", "Augment",
           "white_fill", "FormulaStore", "PageStore", "DeviceDataset", "DeviceLoader", "create_data_loaders",
           "loader_settings", "read_split", "decode_pages_device", "parse_png", "PngInfo"]
