"""The definition of zonal statistics (DESIGN.md "Zonal statistics") in NumPy, for the tests.

``zones`` holds labels 0 .. Z (0 = in no zone), ``valid`` is process_image_masked's mask.  For zone z, S_z = index[valid & (zones
== z)] and its figures are ``analyze_index``'s on S_z: ``orc.stats_app`` and ``orc.hist50``.  The picture-level part is
``masked_model``; nothing of either is restated here."""
import warnings

import numpy as np

import masked_model as mm
from oracle import index_oracle as orc

FIGURES = ("mean", "median", "min", "max", "coverage")


def check_labels(zones, n_zones=None):
    """-> Z; ValueError for labels outside 0 .. Z, naming how many pixels and the range."""
    zones = np.asarray(zones)
    if n_zones is None:
        n_zones = int(zones.max())
    if not 1 <= n_zones <= 65535:
        raise ValueError(f"n_zones must be 1 to 65535, got {n_zones}")
    bad = int(np.count_nonzero((zones < 0) | (zones > n_zones)))
    if bad:
        raise ValueError(f"{bad} pixels have a label outside 0 .. {n_zones}")
    return n_zones


def zone_figures(values, index_type, want_hist=True):
    """The figures of one zone from its values S_z (float32, any order): a dict with pixels, the five FIGURES, hist, and the
    float64 mean / mean |x| the mean's tolerance is taken from."""
    values = np.asarray(values, dtype=np.float32).ravel()
    nan = float("nan")
    out = {"pixels": int(values.size), "hist": np.zeros(50, dtype=np.int64), "mean64": nan, "meanabs": nan}
    if values.size == 0:
        out.update(dict.fromkeys(FIGURES, nan))
        return out
    _, threshold = orc.coverage_rule(index_type)
    finite = values[~np.isnan(values)]
    if want_hist:
        out["hist"] = orc.hist50(finite).astype(np.int64)
    if finite.size != values.size:
        # lars_d_array_stats_f32 / api._summary: NaN mean, median, min and max; NaN > threshold is False, the count includes it
        out.update(dict.fromkeys(FIGURES, nan))
        out["coverage"] = float(np.count_nonzero(finite > np.float32(threshold)) / values.size * 100)
        return out
    st = orc.stats_app(values, index_type)
    feature, _ = orc.coverage_rule(index_type)
    out.update(mean=st[f"Mean {index_type}"], median=st[f"Median {index_type}"], min=st[f"Min {index_type}"], max=st[f"Max {index_type}"],
               coverage=st[f"{feature} Coverage (%)"])
    out["mean64"] = float(np.mean(values.astype(np.float64)))
    out["meanabs"] = float(np.mean(np.abs(values.astype(np.float64))))
    return out


def zonal_model(plane, zones, index_type, valid=None, n_zones=None):
    """``zonal_statistics`` of one float32 plane: a list with one ``zone_figures`` dict per zone 1 .. Z.  One stable argsort of the
    labels, then a split: a single pass however many zones there are."""
    plane = np.asarray(plane, dtype=np.float32)
    zones = np.asarray(zones)
    nz = check_labels(zones, n_zones)
    lab = zones.astype(np.int64).ravel()
    if valid is not None:
        lab = np.where(np.asarray(valid).ravel() != 0, lab, 0)
    order = np.argsort(lab, kind="stable")
    ends = np.searchsorted(lab[order], np.arange(nz + 1), side="right")          # ends[z]: first position after label z
    flat = plane.ravel()[order]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [zone_figures(flat[ends[z - 1]:ends[z]], index_type) for z in range(1, nz + 1)]


def zones_model(img, zones, valid, indices=mm.INDEX_NAMES, white_balance=True, n_zones=None):
    """``process_image_zones``: masked_model's dict (``valid`` is the boolean mask valid_rule derived) plus ``zones`` = {t: list of
    zone_figures}.  The planes are the masked picture's, so the white balance is the picture's, not the plot's."""
    out = mm.masked_model(img, valid, indices, white_balance)
    out["zones"] = {t: zonal_model(out["indices"][t]["index"], zones, t, valid, n_zones) for t in indices}
    return out


def check_zone_figures(got, want, index_type, want_hist=True):
    """``zonal_statistics``'s dict of arrays (or one index's part of ``process_image_zones``'s ``zones`` with ``pixels`` / ``zone``
    merged in) against the model's list: everything exact, the mean within 1e-6 of max(|mean|, mean|x|) of the float64 mean."""
    nz = len(want)
    assert np.array_equal(got["zone"], np.arange(1, nz + 1))
    assert got["pixels"].dtype == np.int64 and np.array_equal(got["pixels"], [w["pixels"] for w in want])
    for f in FIGURES:
        assert got[f].dtype == np.float64 and got[f].shape == (nz,), f
    for f in ("median", "min", "max", "coverage"):
        exp = np.array([w[f] for w in want], dtype=np.float64)
        same = (got[f] == exp) | (np.isnan(got[f]) & np.isnan(exp))
        assert same.all(), (index_type, f, np.flatnonzero(~same)[:5] + 1, got[f][~same][:5], exp[~same][:5])
    for z, w in enumerate(want):
        if np.isnan(w["mean"]):
            assert np.isnan(got["mean"][z]), (index_type, z + 1)
        else:
            assert abs(got["mean"][z] - w["mean64"]) <= 1e-6 * max(abs(w["mean64"]), w["meanabs"]), (index_type, z + 1, got["mean"][z], w["mean64"])
    if want_hist:
        assert got["hist"].dtype == np.int64
        assert np.array_equal(got["hist"], np.array([w["hist"] for w in want]).reshape(nz, 50)), index_type
