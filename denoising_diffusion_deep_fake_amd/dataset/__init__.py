from .image_dataset import ImageDataset, SyntheticFaceDataset, synthetic_face_crops  # noqa: F401
from .device_pool import DeviceImagePool  # noqa: F401
from .balanced import BalancedSampler  # noqa: F401
