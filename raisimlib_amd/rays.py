"""Ray patterns for BatchedWorld.ray_scan (rsb_ray_scan in include/rsb.h): unit directions [P, 3] float32 in the axes of the body that carries the
sensor - x forward, y left, z up.  Pure numpy.  A sensor tilted against its body rotates its pattern once: `dirs @ R.T` with R the sensor's
orientation in the body frame."""
import numpy as np


def depth_camera_rays(width, height, hfov):
    """A pinhole camera looking along +x: one direction through the centre of each pixel of a width x height image, row-major (row 0 is the top
    row, column 0 the left one), square pixels, hfov the horizontal field of view in radians (0 < hfov < pi).  With ray_scan(..., planar=True) the
    ranges are the depth image."""
    width, height, hfov = int(width), int(height), float(hfov)
    if width < 1 or height < 1 or not 0.0 < hfov < np.pi:
        raise ValueError("depth_camera_rays: width and height must be at least 1, hfov inside (0, pi)")
    focal = 0.5 * width / np.tan(0.5 * hfov)                 # in pixels
    u = np.arange(width) + 0.5 - 0.5 * width                 # to the right of the optical axis
    v = np.arange(height) + 0.5 - 0.5 * height               # below it
    d = np.empty((height, width, 3))
    d[..., 0] = focal
    d[..., 1] = -u[None, :]
    d[..., 2] = -v[:, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d.reshape(-1, 3).astype(np.float32)


def lidar_rays(n_azimuth, elevations):
    """A spinning lidar: for each elevation angle (radians above the body's xy plane, in the order given) n_azimuth directions evenly spaced
    around +z, from +x counter-clockwise seen from above: [len(elevations) * n_azimuth, 3], ring by ring."""
    n_azimuth = int(n_azimuth)
    el = np.atleast_1d(np.asarray(elevations, np.float64))
    if n_azimuth < 1 or el.ndim != 1 or el.size < 1:
        raise ValueError("lidar_rays: n_azimuth must be at least 1, elevations a non-empty list of angles")
    az = 2.0 * np.pi * np.arange(n_azimuth) / n_azimuth
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.sin(el)[:, None] * np.ones_like(az)[None, :]], axis=-1)
    return d.reshape(-1, 3).astype(np.float32)
