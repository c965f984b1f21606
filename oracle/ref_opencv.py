"""OpenCV 2.4.5 stand-in under oracle/_ref/.  TEST INFRASTRUCTURE ONLY.

The reference tree ships prebuilt x86-64 OpenCV 2.4.5 (Thirdparty/EDLines/libopencv_core.so.2.4.5 and
libopencv_imgproc.so.2.4.5, no headers); its CMakeLists accepts that version (find_package(OpenCV 2.4.3)).  stage()
copies the two libraries into oracle/_ref/ (git-ignored) and adds the SONAME links; nothing else ever reads the
reference tree.  The loader opens the versioned files themselves, never the links: a copy of the tree that drops
symbolic links still loads (imgproc's DT_NEEDED libopencv_core.so.2.4 is matched against the SONAME of the core that
is already loaded).  The tests load OpenCV from oracle/_ref/ only, through the C API wrapped below (CvMat headers over
numpy buffers).

An OpenCV error is a C++ exception thrown through the C API, which ends the process with terminate(): every wrapper
checks shapes, types and steps in Python before it calls the library.

What this pins: cv::fastAtan2, cvSobel(CV_SCHARR) + cvCartToPolar, cvCvtColor, cvUndistort2, cvCopyMakeBorder, cvGEMM,
cvInvert and cvConvertScale of OpenCV 2.4.5 (tests/test_opencv_pin.py, tests/test_gpu_opencv_pin.py).  OpenCV 3.x is not
on hand and stays unverified.
"""
import ctypes as C
import os
import shutil

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
# where the reference tree is checked out; only stage() looks there
REFERENCE = os.environ.get("SDM_REFERENCE_DIR", "/root/reference")
LIBS = {"libopencv_core.so.2.4.5": "libopencv_core.so.2.4",
        "libopencv_imgproc.so.2.4.5": "libopencv_imgproc.so.2.4"}
CORE = os.path.join(REF_DIR, "libopencv_core.so.2.4.5")
IMGPROC = os.path.join(REF_DIR, "libopencv_imgproc.so.2.4.5")
VERSION = "2.4.5"


def stage(reference=None, verbose=True):
    """Copy the prebuilt OpenCV 2.4.5 libraries into oracle/_ref/ and add their SONAME links.  Without the reference
    tree an existing oracle/_ref/ is kept as it is; nothing fails here (the tests do, loudly, if it is missing)."""
    src_dir = os.path.join(reference or REFERENCE, "Thirdparty", "EDLines")
    have = [os.path.join(src_dir, f) for f in LIBS if os.path.isfile(os.path.join(src_dir, f))]
    if len(have) != len(LIBS):
        state = "kept" if staged() else "MISSING: the OpenCV pins will fail"
        if verbose:
            print("ref_opencv: no OpenCV %s under %s; oracle/_ref/ %s" % (VERSION, src_dir, state))
        return REF_DIR if staged() else None
    os.makedirs(REF_DIR, exist_ok=True)
    for f, soname in LIBS.items():
        dst = os.path.join(REF_DIR, f)
        src = os.path.join(src_dir, f)
        if not (os.path.isfile(dst) and os.path.getsize(dst) == os.path.getsize(src) and
                os.path.getmtime(dst) >= os.path.getmtime(src)):
            shutil.copyfile(src, dst)
            os.chmod(dst, 0o755)
        link = os.path.join(REF_DIR, soname)
        if os.path.islink(link) or os.path.exists(link):
            os.remove(link)
        os.symlink(f, link)
    if verbose:
        print("ref_opencv: staged OpenCV %s in %s" % (VERSION, REF_DIR))
    return REF_DIR


def staged():
    return all(os.path.isfile(os.path.join(REF_DIR, f)) for f in LIBS)


# ---- C API ---------------------------------------------------------------------------------------------------------
CV_8U, CV_16S, CV_32F, CV_64F = 0, 3, 5, 6
_DEPTH = {np.dtype(np.uint8): CV_8U, np.dtype(np.int16): CV_16S, np.dtype(np.float32): CV_32F,
          np.dtype(np.float64): CV_64F}
CV_SCHARR = -1
CV_GEMM_A_T, CV_GEMM_B_T, CV_GEMM_C_T = 1, 2, 4
CV_LU = 0
BORDER_REPLICATE, BORDER_REFLECT_101 = 1, 4
COLOR_TO_GRAY = {"bgr": 6, "rgb": 7, "bgra": 10, "rgba": 11}  # CV_BGR2GRAY, CV_RGB2GRAY, CV_BGRA2GRAY, CV_RGBA2GRAY
_CHANNELS = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4}


class _Point(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int)]


class _Scalar(C.Structure):
    _fields_ = [("val", C.c_double * 4)]


class OpenCV:
    """ctypes view of OpenCV 2.4.5's C API, loaded from oracle/_ref/."""

    def __init__(self):
        if not staged():
            raise RuntimeError("oracle/_ref/ holds no OpenCV %s (libopencv_core/imgproc.so.%s): run "
                               "`python __graft_entry__.py` on a machine with the reference tree to stage it"
                               % (VERSION, VERSION))
        # imgproc's DT_NEEDED is core's SONAME libopencv_core.so.2.4: load core first, globally, by its file name; the
        # dynamic loader then resolves imgproc's dependency to it without any link on disk
        self.core = C.CDLL(CORE, mode=C.RTLD_GLOBAL)
        self.imgproc = C.CDLL(IMGPROC, mode=C.RTLD_GLOBAL)
        vp = C.c_void_p
        L, P = self.core, self.imgproc
        L.cvCreateMatHeader.argtypes = [C.c_int, C.c_int, C.c_int]
        L.cvCreateMatHeader.restype = vp
        L.cvSetData.argtypes = [vp, vp, C.c_int]
        L.cvReleaseMat.argtypes = [C.POINTER(vp)]
        L.cvFastArctan.argtypes = [C.c_float, C.c_float]
        L.cvFastArctan.restype = C.c_float
        L.cvCartToPolar.argtypes = [vp, vp, vp, vp, C.c_int]
        L.cvGEMM.argtypes = [vp, vp, C.c_double, vp, C.c_double, vp, C.c_int]
        L.cvInvert.argtypes = [vp, vp, C.c_int]
        L.cvInvert.restype = C.c_double
        L.cvConvertScale.argtypes = [vp, vp, C.c_double, C.c_double]
        P.cvCopyMakeBorder.argtypes = [vp, vp, _Point, C.c_int, _Scalar]
        P.cvSobel.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
        P.cvCvtColor.argtypes = [vp, vp, C.c_int]
        P.cvUndistort2.argtypes = [vp, vp, vp, vp, vp]
        self.fast_arctan = L.cvFastArctan

    # CvMat header over a C-contiguous 2-D (rows, cols) or 3-D (rows, cols, channels) numpy array
    def _mat(self, a):
        if not isinstance(a, np.ndarray) or a.dtype not in _DEPTH:
            raise TypeError("unsupported array %r" % (getattr(a, "dtype", type(a)),))
        if not a.flags["C_CONTIGUOUS"] or a.ndim not in (2, 3) or a.size == 0:
            raise ValueError("need a non-empty C-contiguous 2-D or 3-D array, got %s" % (a.shape,))
        cn = 1 if a.ndim == 2 else a.shape[2]
        if not 1 <= cn <= 4:
            raise ValueError("1 to 4 channels, got %d" % cn)
        rows, cols = a.shape[:2]
        step = cols * cn * a.itemsize
        if a.strides[0] != step or rows * step >= 2 ** 31:
            raise ValueError("row step %d does not fit a CvMat" % a.strides[0])
        hdr = self.core.cvCreateMatHeader(rows, cols, _DEPTH[a.dtype] + ((cn - 1) << 3))
        if not hdr:
            raise RuntimeError("cvCreateMatHeader failed")
        self.core.cvSetData(hdr, a.ctypes.data, step)
        return hdr

    def _call(self, fn, arrays, *tail_and_args):
        hdrs = [self._mat(a) for a in arrays]
        try:
            fn(*hdrs, *tail_and_args)
        finally:
            self._release(hdrs)

    # -- core ---------------------------------------------------------------------------------------------------------
    def cart_to_polar(self, x, y, degrees=True):
        x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
        if x.shape != y.shape or x.ndim != 2:
            raise ValueError("x, y: equal 2-D shapes")
        mag, ang = np.empty_like(x), np.empty_like(x)
        self._call(self.core.cvCartToPolar, (x, y, mag, ang), int(bool(degrees)))
        return mag, ang

    def gemm(self, A, B, alpha=1.0, Cm=None, beta=0.0, flags=0):
        """cvGEMM: D = alpha * op(A) op(B) + beta * op(C), float32 or float64 matrices"""
        A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
        if A.dtype not in (np.float32, np.float64) or B.dtype != A.dtype or A.ndim != 2 or B.ndim != 2:
            raise TypeError("A, B: 2-D float32/float64 of one type")
        a = A.T if flags & CV_GEMM_A_T else A
        b = B.T if flags & CV_GEMM_B_T else B
        if a.shape[1] != b.shape[0]:
            raise ValueError("inner dimensions %s x %s" % (a.shape, b.shape))
        shape = (a.shape[0], b.shape[1])
        if Cm is not None:
            Cm = np.ascontiguousarray(Cm)
            c = Cm.T if flags & CV_GEMM_C_T else Cm
            if Cm.dtype != A.dtype or c.shape != shape:
                raise ValueError("C must be %s %s" % (A.dtype, shape))
        elif flags & CV_GEMM_C_T:
            raise ValueError("C_T without C")
        D = np.empty(shape, A.dtype)
        hs = [self._mat(A), self._mat(B), self._mat(Cm) if Cm is not None else None, self._mat(D)]
        try:
            self.core.cvGEMM(hs[0], hs[1], alpha, hs[2], beta, hs[3], flags)
        finally:
            self._release(hs)
        return D

    def _release(self, hdrs):
        for h in hdrs:
            if h is not None:
                self.core.cvReleaseMat(C.byref(C.c_void_p(h)))

    def invert(self, A):
        """cvInvert(CV_LU) of a square float32/float64 matrix; returns (inverse, the determinant it reports)"""
        A = np.ascontiguousarray(A)
        if A.dtype not in (np.float32, np.float64) or A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("square float32/float64 matrix")
        D = np.empty_like(A)
        hs = [self._mat(A), self._mat(D)]
        try:
            det = self.core.cvInvert(hs[0], hs[1], CV_LU)
        finally:
            self._release(hs)
        return D, det

    def convert_scale(self, X, scale, shift=0.0):
        """cvConvertScale into the same type: X * scale + shift"""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64) or X.ndim != 2:
            raise ValueError("2-D float32/float64")
        D = np.empty_like(X)
        self._call(self.core.cvConvertScale, (X, D), C.c_double(scale), C.c_double(shift))
        return D

    def copy_make_border(self, src, top, bottom, left, right, border):
        src = np.ascontiguousarray(src)
        if src.ndim != 2 or min(top, bottom, left, right) < 0 or border not in (BORDER_REPLICATE, BORDER_REFLECT_101):
            raise ValueError("2-D source, non-negative margins, REPLICATE or REFLECT_101")
        H, W = src.shape
        dst = np.empty((H + top + bottom, W + left + right), src.dtype)
        self._call(self.imgproc.cvCopyMakeBorder, (src, dst), _Point(left, top), border, _Scalar())
        return dst

    # -- imgproc ------------------------------------------------------------------------------------------------------
    def scharr(self, im):
        """cvSobel(aperture CV_SCHARR) of a gray u8 image into float32: the integer sums (sx, sy), replicated border"""
        im = np.ascontiguousarray(im)
        if im.dtype != np.uint8 or im.ndim != 2:
            raise ValueError("gray uint8 image")
        sx, sy = np.empty(im.shape, np.float32), np.empty(im.shape, np.float32)
        self._call(self.imgproc.cvSobel, (im, sx), 1, 0, CV_SCHARR)
        self._call(self.imgproc.cvSobel, (im, sy), 0, 1, CV_SCHARR)
        return sx, sy

    def cvt_gray(self, px, order):
        """cvCvtColor(<order>2GRAY) of an interleaved u8 frame"""
        px = np.ascontiguousarray(px)
        if order not in COLOR_TO_GRAY or px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != _CHANNELS[order]:
            raise ValueError("u8 frame (H, W, %s) for %r" % (_CHANNELS.get(order), order))
        gray = np.empty(px.shape[:2], np.uint8)
        self._call(self.imgproc.cvCvtColor, (px, gray), COLOR_TO_GRAY[order])
        return gray

    def undistort(self, px, K, dist):
        """cvUndistort2 (cv::undistort) of a 1/3/4-channel u8 frame; K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3),
        both float32 as Tracking holds them (src/Tracking.cc:52-75)"""
        px = np.ascontiguousarray(px)
        if px.dtype != np.uint8 or px.ndim not in (2, 3) or (px.ndim == 3 and px.shape[2] not in (3, 4)):
            raise ValueError("u8 frame of 1, 3 or 4 channels")
        fx, fy, cx, cy = np.asarray(K, np.float32).ravel()
        Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
        d = np.ascontiguousarray(np.asarray(dist, np.float32).reshape(5, 1))
        out = np.empty_like(px)
        hs = [self._mat(px), self._mat(out), self._mat(Km), self._mat(d)]
        try:
            self.imgproc.cvUndistort2(hs[0], hs[1], hs[2], hs[3], None)
        finally:
            self._release(hs)
        return out


_LOADED = None


def load():
    """the process-wide OpenCV 2.4.5 handle; raises (never skips) when oracle/_ref/ is not staged"""
    global _LOADED
    if _LOADED is None:
        _LOADED = OpenCV()
    return _LOADED
