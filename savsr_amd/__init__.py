"""savsr_amd -- MI355X-native SAVSR inference path."""
from .registry import ARCH_REGISTRY, DATASET_REGISTRY, METRIC_REGISTRY, MODEL_REGISTRY  # noqa: F401
from .archs import build_network  # noqa: F401
from .archs.savsr_arch import SAVSR  # noqa: F401
from . import datasets as _datasets, models as _models  # noqa: F401,E402  (register ASVideoTestDataset / ASVSRModel)
from .datasets import build_dataset  # noqa: F401,E402
from .models import build_model  # noqa: F401,E402
from .video import (GridVerdict, NoiseVerdict, ScanStats, ScanVerdict, VideoUpscaler, comb_windows, deblock_video, denoise_spatial, denoise_video, dering_video, detect_active_area, detect_cuts,  # noqa: F401,E402
                    detect_grid, detect_scan, estimate_noise, field_scores, field_stats, grid_stats, line_sums, noise_stats, pack_surface, pair_sad, remove_pulldown, unpack_surface)
from . import denoise  # noqa: F401,E402  (the specification of denoise_video / upscale_video(denoise=...))
from . import nlmeans  # noqa: F401,E402  (the specification of denoise_spatial / upscale_video(spatial_denoise=...))
from . import dering  # noqa: F401,E402  (the specification of dering_video / upscale_video(dering=...))
from . import deblock  # noqa: F401,E402  (the specification of deblock_video / upscale_video(deblock=...))
from . import grid  # noqa: F401,E402  (the specification of grid_stats / detect_grid / upscale_video(deblock_grid="auto"))
from . import noise  # noqa: F401,E402  (the specification of noise_stats / estimate_noise / upscale_video(denoise_strength="auto", spatial_strength="auto"))
from . import dither  # noqa: F401,E402  (the specification of upscale_video(dither=...) and the `_d` quantiser entries)
from . import scan  # noqa: F401,E402  (the specification of field_stats / detect_scan / upscale_video(scan="detect"))
from . import surface  # noqa: F401,E402  (the specification of unpack_surface / pack_surface / upscale_video(surface=..., out_surface=...))
from .surface import Surface  # noqa: F401,E402
from . import pulldown  # noqa: F401,E402  (the specification of remove_pulldown / upscale_video(pulldown=...))
from . import deinterlace  # noqa: F401,E402  (the specification module; calling it is savsr_amd.video.deinterlace, the GPU function)

__version__ = "0.1.0"
