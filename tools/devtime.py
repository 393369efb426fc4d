"""The event timer of the *_time.py tools: a call timed on the device with the library's event hooks (s5gpu_event_*).

  timed(L, fn, reps, warm=2) -> (median ms, least ms) of `reps` calls of fn() after `warm` untimed ones
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib  # noqa: E402


def timed(L, fn, reps, warm=2):
    vp = C.c_void_p
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1, t = vp(), vp(), C.c_float()
        _lib.check(L.s5gpu_event_create(C.byref(e0))); _lib.check(L.s5gpu_event_create(C.byref(e1)))
        _lib.check(L.s5gpu_event_record(e0, None))
        fn()
        _lib.check(L.s5gpu_event_record(e1, None))
        _lib.check(L.s5gpu_event_elapsed_ms(e0, e1, C.byref(t)))
        _lib.check(L.s5gpu_event_destroy(e0)); _lib.check(L.s5gpu_event_destroy(e1))
        ms.append(t.value)
    return float(np.median(ms)), float(min(ms))
