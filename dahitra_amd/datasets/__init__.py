from .xbd_pipeline import GpuXbdPipeline, draw_train_params, resize_coeffs  # noqa: F401
