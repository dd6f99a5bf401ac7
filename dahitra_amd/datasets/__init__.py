from .xbd_pipeline import (GpuXbdPipeline, draw_jitter_params, draw_train_params, draw_unet_colour, draw_unet_noise,  # noqa: F401
                           draw_unet_params, jitter_reference_u8, resize_coeffs, split_indices, train_indices,
                           unet_colour_reference_u8, unet_reference_u8, unet_train_indices, unet_warp_table, warp_affine_u8)
