"""Data helpers on the path's kernels: the dataset's numpy farthest point sampling, host-to-device
prefetching, and the device-resident dataset + loader (device_loader.py)."""
from .dataset_3d import farthest_point_sample, pc_normalize  # noqa: F401
from .prefetch import DevicePrefetcher  # noqa: F401
from .fps_service import start_fps_service, stop_fps_service  # noqa: F401
from .device_loader import DeviceCloudSet, DeviceBatchLoader, epoch_indices, numpy_draws  # noqa: F401
from .augment import (rotate_point_cloud, random_point_dropout, random_scale_point_cloud, shift_point_cloud,  # noqa: F401
                      jitter_point_cloud, rotate_perturbation_point_cloud)
from .fewshot import fewshot_indices  # noqa: F401
