from .transforms import (Compose, Resize, RandomHorizontalFlip, ToTensor, Normalize, AdjustBrightness, AdjustContrast,
                         AdjustHue, RandomErasing, DeviceImage, augment_views, tta_views)
from .build import build_transforms

__all__ = ["Compose", "Resize", "RandomHorizontalFlip", "ToTensor", "Normalize", "AdjustBrightness", "AdjustContrast",
           "AdjustHue", "RandomErasing", "DeviceImage", "augment_views", "tta_views", "build_transforms"]
