from .xbd_pipeline import (GpuXbdPipeline, draw_jitter_params, draw_train_params, draw_unet_params,  # noqa: F401
                           jitter_reference_u8, resize_coeffs, unet_reference_u8, unet_warp_table, warp_affine_u8)
