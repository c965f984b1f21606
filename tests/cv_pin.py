"""Helpers of the OpenCV 2.4.5 pins (tests/test_opencv_pin.py, tests/test_gpu_opencv_pin.py,
tests/golden/make_fastatan2_digest.py): the staged library, the committed calibrations, and a small threaded C harness
that walks cv::fastAtan2(y, 1) against the oracle's pmo_fast_atan2 over float bit patterns.

The harness is compiled at test time against oracle/_build/libpm_oracle.so and dlopen()s the staged
oracle/_ref/libopencv_core.so.2.4.5.  Its digest is the order-independent sum (mod 2^64) over the walked patterns i of
mix64(i << 32 | bits(cvFastArctan(y_i, 1))), NaN results canonicalised to 0x7fc00000; sdm_selftest(10) computes the same
sum on the device from K1's fast_atan2_deg_x1."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_THREADS = 16

_SRC = r"""
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>

float pmo_fast_atan2(float y, float x);
typedef float (*atan_fn)(float, float);

static uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;  /* SplitMix64 finaliser */
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float bitsf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

typedef struct { atan_fn cv; uint64_t lo, hi, stride; uint64_t bad, digest, first_bad; } job;

static void *run(void *p)
{
    job *j = (job *)p;
    uint64_t bad = 0, dig = 0, first = ~0ull;
    for (uint64_t i = j->lo; i < j->hi; i += j->stride) {
        const float y = bitsf((uint32_t)i);
        const float a = j->cv(y, 1.0f), b = pmo_fast_atan2(y, 1.0f);
        const int na = a != a, nb = b != b;
        if (!(fbits(a) == fbits(b) || (na && nb))) { if (!bad) first = i; bad++; }
        dig += mix64((i << 32) | (na ? 0x7fc00000u : fbits(a)));
    }
    j->bad = bad; j->digest = dig; j->first_bad = first;
    return 0;
}

/* walk lo, lo+stride, ... < hi on `threads` threads; returns mismatches (-1: no OpenCV), adds to *digest */
long long sweep_x1(const char *core, uint64_t lo, uint64_t hi, uint64_t stride, int threads, uint64_t *digest,
                   uint64_t *first_bad)
{
    void *h = dlopen(core, RTLD_NOW | RTLD_GLOBAL);
    if (!h) return -1;
    atan_fn cv = (atan_fn)dlsym(h, "cvFastArctan");
    if (!cv || threads < 1 || threads > 16 || stride == 0 || hi <= lo) return -1;
    const uint64_t n = (hi - lo + stride - 1) / stride, per = (n + threads - 1) / threads;
    job jobs[16];
    pthread_t tid[16];
    for (int t = 0; t < threads; t++) {
        const uint64_t a = t * per, b = (t + 1) * per < n ? (t + 1) * per : n;
        jobs[t].cv = cv; jobs[t].lo = lo + a * stride; jobs[t].hi = a < b ? lo + (b - 1) * stride + 1 : jobs[t].lo;
        jobs[t].stride = stride; jobs[t].bad = 0; jobs[t].digest = 0; jobs[t].first_bad = ~0ull;
        if (pthread_create(&tid[t], 0, run, &jobs[t]) != 0) run(&jobs[t]), tid[t] = 0;
    }
    long long bad = 0;
    for (int t = 0; t < threads; t++) {
        if (tid[t]) pthread_join(tid[t], 0);
        bad += (long long)jobs[t].bad;
        *digest += jobs[t].digest;
        if (jobs[t].first_bad < *first_bad) *first_bad = jobs[t].first_bad;
    }
    return bad;
}

/* the oracle's fast_atan2 over arrays (the GradTheta of any (gx, gy)) */
void oracle_atan2(const float *y, const float *x, float *out, long long n)
{
    for (long long i = 0; i < n; i++) out[i] = pmo_fast_atan2(y[i], x[i]);
}
"""


def opencv():
    """OpenCV 2.4.5 from oracle/_ref/ -- raises (never skips) when it is not staged"""
    import ref_opencv
    return ref_opencv.load()


def calibrations():
    """the reference's camera calibrations (tests/golden/calibrations.json): (source, W, H, K float32[4], dist float32[5])"""
    with open(os.path.join(GOLDEN, "calibrations.json")) as f:
        doc = json.load(f)
    return [(c["source"], c["W"], c["H"], np.float32([float(v) for v in c["K"]]),
             np.float32([float(v) for v in c["dist"]])) for c in doc["calibrations"]]


def _c_compiler():
    for cc in ("cc", "gcc", "clang"):
        p = shutil.which(cc)
        if p:
            return p
    raise RuntimeError("no C compiler for the fastAtan2 harness")


class Harness:
    def __init__(self, out_dir):
        import pm_oracle
        import ref_opencv
        opencv()  # staged and loadable, or raise here
        self.core = ref_opencv.CORE  # the versioned file, the one ref_opencv loaded (no SONAME link needed)
        lib_oracle = pm_oracle.build("strict")
        src = os.path.join(out_dir, "cv_pin_harness.c")
        so = os.path.join(out_dir, "cv_pin_harness.so")
        with open(src, "w") as f:
            f.write(_SRC)
        odir = os.path.dirname(lib_oracle)
        subprocess.check_call([_c_compiler(), "-std=gnu99", "-O2", "-fPIC", "-shared", src, "-o", so,
                               "-L" + odir, "-Wl,-rpath," + odir, "-lpm_oracle", "-ldl", "-lpthread"])
        L = self.lib = C.CDLL(so)
        u64 = C.c_uint64
        L.sweep_x1.argtypes = [C.c_char_p, u64, u64, u64, C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.sweep_x1.restype = C.c_longlong
        L.oracle_atan2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        self.threads = max(1, min(MAX_THREADS, os.cpu_count() or 1))

    def sweep(self, lo, hi, stride=1):
        """(mismatches, digest, first mismatching pattern or None) over the patterns lo, lo + stride, ... < hi"""
        dig, first = C.c_uint64(0), C.c_uint64(2 ** 64 - 1)
        bad = self.lib.sweep_x1(self.core.encode(), lo, hi, stride, self.threads, C.byref(dig), C.byref(first))
        if bad < 0:
            raise RuntimeError("fastAtan2 harness could not load cvFastArctan from " + self.core)
        return bad, dig.value, (None if first.value == 2 ** 64 - 1 else first.value)

    def all_patterns(self):
        """every one of the 2^32 patterns: (mismatches, digest)"""
        bad, dig = 0, 0
        for lo in range(0, 2 ** 32, 2 ** 30):
            b, d, _ = self.sweep(lo, lo + 2 ** 30)
            bad, dig = bad + b, (dig + d) % 2 ** 64
        return bad, dig

    def oracle_atan2(self, y, x):
        y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
        assert y.shape == x.shape
        out = np.empty_like(y)
        self.lib.oracle_atan2(y.ctypes.data, x.ctypes.data, out.ctypes.data, y.size)
        return out


def digest_fixture():
    with open(os.path.join(GOLDEN, "fastatan2_x1_digest.json")) as f:
        return json.load(f)
