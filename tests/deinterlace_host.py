"""csrc/deinterlace.hip's sample code run on the host: the file builds alone, with SWK_DEINT_HOST_CHECK set, into a shared object whose
swk_deint_plane_host walks one plane sample group by sample group through the very function the kernel calls (deint_quad).  No GPU
is touched: the object only holds the kernel beside the host code."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DeintPlane(ctypes.Structure):          # csrc/swk_internal.h
    _fields_ = [("src", ctypes.c_void_p), ("fs", ctypes.c_int64), ("rs", ctypes.c_int64), ("step", ctypes.c_int), ("oy", ctypes.c_int),
                ("ox", ctypes.c_int), ("PH", ctypes.c_int), ("PW", ctypes.c_int), ("py0", ctypes.c_int), ("px0", ctypes.c_int),
                ("ph", ctypes.c_int), ("pw", ctypes.c_int), ("parity0", ctypes.c_int), ("msb", ctypes.c_int), ("dst", ctypes.c_void_p)]


class DeintJob(ctypes.Structure):
    _fields_ = [("count", ctypes.c_int), ("first", ctypes.c_int), ("nout", ctypes.c_int), ("rate", ctypes.c_int), ("tff", ctypes.c_int),
                ("temporal", ctypes.c_int)]


def build(outdir):
    csrc = os.path.join(ROOT, "swiftwatcher_amd", "csrc")
    lib = os.path.join(str(outdir), "libdeint_host.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DSWK_DEINT_HOST_CHECK",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-shared", os.path.join(csrc, "deinterlace.hip"), "-o", lib])
    lib = ctypes.CDLL(lib)
    check_layout(lib)
    return lib


def check_layout(lib):
    """the ctypes mirrors above against the structs as compiled (swk_deint_layout): sizes and every member's offset"""
    got = (ctypes.c_int * 64)()
    n = lib.swk_deint_layout(got, 64)
    mine = [ctypes.sizeof(DeintPlane), ctypes.sizeof(DeintJob)] + [getattr(DeintPlane, f).offset for f, _ in DeintPlane._fields_] + \
           [getattr(DeintJob, f).offset for f, _ in DeintJob._fields_]
    assert list(got[:n]) == mine, "csrc/swk_internal.h's DeintPlane / DeintJob and their ctypes mirrors differ: %s != %s" % (list(got[:n]), mine)


def plane(lib, stored, rect, *, tff, rate=2, temporal=True, has_prev=False, has_next=False, parity0=0, step=1, which=0, msb=0,
          staged=False):
    """One plane through the host build.  stored: (count, PH, PW) uint8 / uint16 words as they lie in memory, or (count, PH, PW, 2)
    with step=2 (interleaved chroma; which = 0 / 1 picks U / V).  rect = (px0, py0, pw, ph) in plane coordinates.  staged: hand over
    only the rectangle grown by the footprint, as the library stages a host source.  Returns (nout, ph, pw) LSB-aligned samples."""
    stored = np.ascontiguousarray(stored)
    B = stored.dtype.itemsize
    spare = 4 // B                                   # (the aligned-dword path reads up to 3 bytes on either side of a row's samples)
    count, PH, PW = stored.shape[:3]
    px0, py0, pw, ph = rect
    oy = ox = 0
    held = stored
    if staged:
        oy, ox = max(py0 - 1, 0), max(px0 - 3, 0)
        held = np.ascontiguousarray(stored[:, oy:min(py0 + ph + 1, PH), ox:min(px0 + pw + 3, PW)])
    room = np.zeros(held.size + 2 * spare, held.dtype)
    room[spare:spare + held.size] = held.reshape(-1)
    held = room[spare:spare + held.size].reshape(held.shape)
    first, nframes = int(bool(has_prev)), count - int(bool(has_prev)) - int(bool(has_next))
    nout = rate * nframes
    guard = 8
    out = np.full(nout * ph * pw + 2 * guard, 0xA5A5 if B == 2 else 0xA5, stored.dtype)
    p = DeintPlane(src=held.ctypes.data + which * B, fs=held.strides[0], rs=held.strides[1], step=step, oy=oy, ox=ox, PH=PH, PW=PW, py0=py0,
                   px0=px0, ph=ph, pw=pw, parity0=parity0, msb=msb, dst=out.ctypes.data + guard * B)
    j = DeintJob(count=count, first=first, nout=nout, rate=rate, tff=int(bool(tff)), temporal=int(bool(temporal)))
    lib.swk_deint_plane_host(ctypes.byref(p), ctypes.byref(j), int(B == 2))
    assert (out[:guard] == out[0]).all() and (out[-guard:] == out[0]).all(), "the host build wrote outside its output"
    return out[guard:-guard].reshape(nout, ph, pw)
