from .xbd_pipeline import (GpuXbdPipeline, draw_jitter_params, draw_train_params, jitter_reference_u8,  # noqa: F401
                           resize_coeffs)
