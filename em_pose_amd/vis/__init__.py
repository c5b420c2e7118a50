"""Headless visualisation: cameras, the HIP mesh renderer, overlays drawn into its frames and image output."""
from em_pose_amd.vis.camera import Camera, fit_camera, look_at, pinhole  # noqa: F401
from em_pose_amd.vis.io import contact_sheet, save_frames, save_image, side_by_side  # noqa: F401
from em_pose_amd.vis.renderer import MeshRenderer, error_colors  # noqa: F401
from em_pose_amd.vis.overlay import (Primitives, draw_primitives, residual_primitives, sensor_primitives,  # noqa: F401
                                     skeleton_primitives)
