"""`from models.tiles import predict_tiles` ...: whole-tile change maps under the reference's package name"""
from dahitra_amd.models.tiles import TilePlan, evaluate_tiles, forget_tile_steps, predict_tile, predict_tiles  # noqa: F401
