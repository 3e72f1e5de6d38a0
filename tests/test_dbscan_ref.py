"""DBScan keypoint thinning, CPU side: the numpy restatement (tests/dbscan_ref_py.py) equals the reference's own dbscan.cpp on
every case of tests/golden/dbscan_reference.npz, and the library's square-domain bound of the neighbour predicate
(ps_debug_dbscan_bound) equals an independent bisection for every kind of eps."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dbscan_ref_py as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "dbscan_reference.npz")


def golden_cases():
    z = np.load(GOLDEN)
    off, koff = z["offsets"], z["kept_offsets"]
    for c in range(len(off) - 1):
        yield (z["xy"][off[c]:off[c + 1]], z["octave"][off[c]:off[c + 1]], float(z["eps"][c]), int(z["min_pts"][c]),
               int(z["features_from_cluster"][c]), z["kept"][koff[c]:koff[c + 1]])


def test_golden_covers_the_contract():
    cs = list(golden_cases())
    assert len(cs) >= 300
    ns = [len(c[0]) for c in cs]
    assert max(ns) == 5000 and 0 in ns and 1 in ns
    assert {0.0, 0.5, 1.0, 1.5, 2.0} <= {c[2] for c in cs}
    assert any(np.isnan(c[2]) for c in cs) and any(c[2] < 0 for c in cs)
    assert {0, 1, 2, 3, 4} <= {c[3] for c in cs} and {0, 1, 2, 3} <= {c[4] for c in cs}
    assert any((c[1] == -5).any() for c in cs) and any(np.isnan(c[0]).any() for c in cs)
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_restatement_equals_reference_binary():
    bad = []
    for i, (xy, octave, eps, mp, ffc, kept) in enumerate(golden_cases()):
        got = R.dbscan_keep(xy, octave, eps, mp, ffc)
        if not np.array_equal(got, kept):
            bad.append((i, len(xy), eps, mp, ffc))
    assert not bad, bad[:10]


def _eps_sweep():
    rng = np.random.default_rng(7)
    tiny = [5e-324, 1e-320, 2.2250738585072014e-308, 1e-300, 1.4e-45, 1e-40, 1e-30]
    huge = [1e30, 1.8446742974197924e19, 3.4028234663852886e38, 3.4028235677973366e38, 1e39, 1e300, 1.7976931348623157e308]
    plain = [0.1, 0.5, 1.0, 1.5, 2.0, 3.0, 10.0, 0.75, 1.0 + 2 ** -52, 1.0 - 2 ** -53, float(np.float32(0.1))]
    special = [0.0, -0.0, -1.0, -1e-300, float("nan"), float("inf"), float("-inf")]
    rand = list(10.0 ** rng.uniform(-8, 8, 40)) + list(np.float32(rng.uniform(0, 20, 20)).astype(np.float64))
    return tiny + huge + plain + special + rand


def test_dbscan_bound_equals_bisection():
    from putslam_amd import api
    for eps in _eps_sweep():
        got, want = api.dbscan_bound(eps), R.dbscan_bound(eps)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (eps, got, want)


def test_dbscan_bound_is_the_predicate():
    """s < bound(eps) decides (double)(float)sqrt(s) < eps at the bound and at its neighbours."""
    from putslam_amd import api
    with np.errstate(all="ignore"):
        for eps in _eps_sweep():
            b = api.dbscan_bound(eps)
            for s in (b, np.nextafter(b, 0.0), np.nextafter(b, np.inf), 0.0):
                if not np.isfinite(s):
                    continue
                assert (float(np.float32(np.sqrt(s))) < eps) == (s < b), (eps, s, b)


def test_bad_arguments_fail_without_a_gpu_call():
    """ps_dbscan_thin* reject a null context before anything else (PS_ERR_BAD_ARG)."""
    import ctypes
    from putslam_amd import _lib
    L = _lib.load()
    n = ctypes.c_int(5)
    assert L.ps_dbscan_thin(None, None, 8, None, 4, 0, 1.0, 2, 1, None, ctypes.byref(n)) == -1
    assert L.ps_dbscan_thin_device(None, None, None, None, 0, 1, 1.0, 2, 1, None, None) == -1


def test_dropin_defines_dbscan():
    so = os.path.join(ROOT, "putslam_amd", "libputslam_dropin.so")
    if not os.path.exists(so):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build_dropin()
    names = subprocess.check_output("nm -D --defined-only %s | c++filt" % so, shell=True, text=True)
    assert "DBScan::run(std::vector<cv::KeyPoint" in names
    assert "DBScan::DBScan(double, int, int)" in names


# the interface of the reference's include/putslam/Matcher/dbscan.h (signatures, data members, include guard), as a translation
# unit compiled against it declares the class
_REFERENCE_SHAPED_DBSCAN_H = """#ifndef _DBSCAN
#define _DBSCAN
#include <vector>
class DBScan {
public:
    DBScan(double eps = 10, int minPts = 2, int featuresFromCluster = 1);
    void run(std::vector<cv::KeyPoint> &clusteringSet);
private:
    double eps;
    int minPts;
    int featuresFromCluster;
    std::vector<std::vector<float> > dist;
    std::vector<bool> visited;
    std::vector<int> cluster;
    void expandCluster(std::vector<int> neighbourList, int clusteringSetSize, int &C);
    int findingClusters(int clusteringSetSize);
};
#endif
"""


@pytest.mark.parametrize("order", ["reference_first", "dropin_first"])
def test_dropin_header_next_to_reference_dbscan_header(tmp_path, order):
    """matcher.cpp includes Matcher/dbscan.h and, through the glue, putslam_dropin.h: one translation unit with both headers, in
    either order, compiles and runs DBScan (the drop-in's class sits behind the reference header's guard)."""
    (tmp_path / "dbscan.h").write_text('#include "putslam_compat_types.h"\n' + _REFERENCE_SHAPED_DBSCAN_H)
    inc = ['#include "dbscan.h"', '#include "putslam_dropin.h"']
    if order == "dropin_first":
        inc.reverse()
    src = tmp_path / "tu.cpp"
    src.write_text("\n".join(inc) + "\nvoid thin(std::vector<cv::KeyPoint> &k) { DBScan d(1.0); d.run(k); }\n"
                   "static_assert(sizeof(DBScan) == sizeof(double) + 2 * sizeof(int) + sizeof(std::vector<std::vector<float> >)"
                   " + sizeof(std::vector<bool>) + sizeof(std::vector<int>), \"layout\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(tmp_path), "-I",
                           os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "putslam_amd", "csrc", "dropin"), str(src)])
