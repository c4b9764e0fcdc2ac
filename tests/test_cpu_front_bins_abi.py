"""Direct bins (tgs.h): the length function, the argument checks of the three _bins entry points -- all before any launch,
so they run without a GPU -- and the host-side rule that decides whether a frame gets bins (ops.FrontBuffers.attach_bins)."""
import ctypes as C

import pytest
import torch


def camera(W=64, H=48):
    from touch_gs_amd import _lib
    cam = _lib.TgsCamera()
    cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy = W, H, 50.0, 50.0, W / 2, H / 2
    for i in (0, 5, 10, 15):
        cam.viewmat[i] = 1.0
    return cam


def test_bins_len():
    from touch_gs_amd import _lib
    lib = _lib.load()
    assert lib.tgs_version() == 320
    assert lib.tgs_bins_len(12, 1022) == 8 * 12 * 1022
    assert lib.tgs_bins_len(8160, 1022) * 8 == 533_729_280            # 1080p, the flagship's bound: 534 MB per frame
    assert lib.tgs_bins_len(65025, 4096) == 8 * 65025 * 4096           # beyond 2^31 entries: 64-bit
    assert lib.tgs_bins_len(0, 10) == 0 and lib.tgs_bins_len(10, 0) == 0 and lib.tgs_bins_len(10, -1) == 0


def test_bins_entry_points_refuse_bad_bins_before_any_launch():
    from touch_gs_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)      # never dereferenced: every check here precedes the first launch
    spec = C.byref(_lib.TgsAdamSpec())
    cam = camera()
    T = lib.tgs_num_tiles(64, 48)
    ts_len = lib.tgs_tile_start_len(64, 48)

    def k8(bins, bins_len, cap):
        return lib.tgs_project_bwd_adam_next_front_bins(C.byref(cam), 256, 16, 3, fake, fake, fake, spec, fake, fake, fake, None,
                                                        None, C.byref(cam), fake, fake, 1, fake, None, fake, fake, 1024, fake,
                                                        fake, None, 0, bins, bins_len, cap, None)

    def finish(bins, bins_len, cap):
        return lib.tgs_project_bin_sort_front_bins(C.byref(cam), 256, fake, fake, fake, fake, fake, 16, 3, fake, None, fake, fake,
                                                   ts_len, fake, fake, None, 1024, fake, fake, None, -1, fake, 0, None, None, None,
                                                   bins, bins_len, cap, None)

    def records(bins, bins_len, cap):
        return lib.tgs_bin_sort_bins(C.byref(cam), 256, fake, fake, fake, ts_len, fake, fake, None, 1024, fake, fake, None, -1,
                                     bins, bins_len, cap, None)

    for call, name in ((k8, b"tgs_project_bwd_adam_next_front_bins"), (finish, b"tgs_project_bin_sort_front_bins"),
                       (records, None)):
        for bins, bins_len, cap in ((fake, lib.tgs_bins_len(T, 100) - 1, 100),     # one entry short
                                    (fake, 0, 100), (fake, -1, 100),
                                    (None, lib.tgs_bins_len(T, 100), 100),           # no buffer
                                    (fake, lib.tgs_bins_len(T, 100), 0),             # no capacity
                                    (fake, lib.tgs_bins_len(T, 100), -5),
                                    (fake, lib.tgs_bins_len(T, 4097), 4097)):        # beyond the register sorts' classes
            rc = call(bins, bins_len, cap)
            msg = lib.tgs_last_error()
            assert rc == -1 and b"tgs_bins_len" in msg, (rc, msg)
            assert name is None or msg.startswith(name + b":"), msg
    # the other checks of the two front entry points still come first, in the caller's name
    rc = lib.tgs_project_bwd_adam_next_front_bins(C.byref(cam), 256, 16, 3, fake, fake, fake, spec, fake, fake, fake, None, None,
                                                  None, fake, fake, 1, fake, None, fake, fake, 1024, fake, fake, None, 0, fake,
                                                  lib.tgs_bins_len(T, 100), 100, None)
    assert rc == -1 and lib.tgs_last_error().startswith(b"tgs_project_bwd_adam_next_front_bins:") and b"next camera" in lib.tgs_last_error()
    rc = lib.tgs_project_bin_sort_front_bins(C.byref(cam), 256, fake, fake, fake, fake, fake, 16, 3, fake, None, fake, fake,
                                             ts_len - 1, fake, fake, None, 1024, fake, fake, None, -1, fake, 0, None, None, None,
                                             fake, lib.tgs_bins_len(T, 100), 100, None)
    assert rc == -1 and b"tgs_tile_start_len" in lib.tgs_last_error()


def test_a_frame_gets_bins_only_under_a_bound_and_the_ceiling():
    from touch_gs_amd import Camera, ops
    import numpy as np
    cam = Camera(np.eye(4), 50.0, 50.0, 32.0, 24.0, 64, 48)
    was = ops.set_front_bins()
    try:
        assert ops.set_front_bins(True, 1 << 30) == (True, 1 << 30)

        def attach(hint, N=300):
            fb = ops.FrontBuffers(cam, N, 4096, False, torch.device("cpu"))
            assert fb.bins is None and fb.bin_cap == 0 and not fb.bins_filled
            got = fb.attach_bins(hint)
            assert got == (fb.bins is not None)
            return fb

        fb = attach(100)
        assert fb.bin_cap == 100 and tuple(fb.bins.shape) == (8 * 12 * 100, 2) and fb.bins.dtype == torch.int32
        assert attach(4096).bin_cap == 4096
        for hint in (-1, 0, 4097):                       # no bound; lists of the `huge` class
            assert attach(hint).bins is None
        assert attach(100, N=0).bins is None
        ops.set_front_bins(max_bytes=8 * 12 * 100 * 8 - 1)            # one byte short of that frame's bins
        assert attach(100).bins is None and attach(99).bins is not None
        ops.set_front_bins(False, 1 << 30)
        assert attach(100).bins is None
    finally:
        ops.set_front_bins(*was)
