"""The table of stream-order cases (tests/stream_order_cases.py) is complete -- every asynchronous entry point of the header has a
case, or stands in EXEMPT with its reason, and is bound in _lib.py -- and the scene of the front-end chain keeps what it was chosen
for: every step removes some rows and not all.  No GPU."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stream_order_cases as S  # noqa: E402

ROOT = os.path.dirname(HERE)


def header_entry_points():
    """Every function of include/putslam_hip.h whose name ends in _device and whose first parameter is `PsContext *`."""
    with open(os.path.join(ROOT, "include", "putslam_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return set(re.findall(r"\b(ps_\w+_device)\s*\(\s*PsContext\s*\*", text))


def test_every_asynchronous_entry_point_has_an_order_case():
    names = header_entry_points()
    assert len(names) >= 23 and "ps_context_device" not in names
    assert not set(S.TABLE) & set(S.EXEMPT)
    assert names == set(S.TABLE) | set(S.EXEMPT), (sorted(names - set(S.TABLE) - set(S.EXEMPT)), sorted((set(S.TABLE) | set(S.EXEMPT)) - names))
    assert len(S.TABLE) == 22 and all(len(reason) > 20 for reason in S.EXEMPT.values())
    assert {n for n, e in S.TABLE.items() if e.drains} == {"ps_map_views_device", "ps_map_views_l2_device", "ps_pose_sets_device",
                                                          "ps_pose_sets_l2_device", "ps_frame_levels_device"}


def test_every_case_is_bound():
    from putslam_amd import _lib
    with open(_lib.__file__) as f:
        text = f.read()
    for name in list(S.TABLE) + list(S.EXEMPT):
        assert name in _lib.EXPORTED and re.search(r"L\.%s\.argtypes" % name, text), name


def test_chain_scene_loses_rows_at_every_step_and_not_all():
    ref, want = S.chain_reference(), S.CHAIN_COUNTS
    fr = ref["frames"]
    assert [len(f["xy"]) for f in fr] == want["detected"] == [128, 128]
    assert [len(f["keep"]) for f in fr] == want["thinned"] == [89, 89]
    assert [len(f["kept"]) for f in fr] == want["described"] == [22, 23]
    assert int(ref["status"].sum()) == want["tracked"] == 87
    assert len(ref["selected"]) == want["selected"] == 57
    good = ref["status"] != 0
    flow = ref["next"][good] - fr[0]["kxy"][good]
    assert abs(float(np.median(flow[:, 0])) - 2.0) < 0.005 and abs(float(np.median(flow[:, 1]))) < 0.005
