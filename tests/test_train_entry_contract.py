"""The argument checks of the training-march entry points (ugrid_train_*), in the order a caller can observe them (no GPU needed):
every case here returns before a kernel launch and before any pointer but `mask_dims3` is read, so the non-null pointers are dummies.

0 = nothing to do (n_rays <= 0), 1 = hipErrorInvalidValue.  One entry point answers out of step with the others and is pinned as it
is: ugrid_train_sample looks at its four stage-2 outputs BEFORE the ray count, so it returns 1 for a null one even with no rays."""
import ctypes

import pytest

PTR = 4096                        # a non-null value: never dereferenced, the checks come first
OUT8 = ("scratch_pts", "scratch_density", "scratch_step", "scratch_w", "scratch_T", "count", "count2", "alphainv_last")
STAGE2 = ("scratch_w", "scratch_T", "count2", "alphainv_last")      # the outputs the entry points look at
MASK = ("mask", "mask_dims3", "xyz2ijk_scale3", "xyz2ijk_shift3")
FOURIER = ("density_grid", "P", "X", "Y", "Z", "freq_num", "rays_o", "rays_d", "n_rays", "t_table", "n_samples", "scene_center3",
           "scene_radius3", "xyz_min", "xyz_max", "bg_len", "norm_l2", "act_shift", "interval", "thres")
DCVGO = ("rays_o", "rays_d", "n_rays", "t_table", "n_samples", "scene_center3", "scene_radius3", "xyz_min", "xyz_max", "bg_len", "norm_l2",
         "dist_thres") + MASK + ("act_shift", "interval", "thres") + OUT8 + ("stream",)
DVGO = ("rays_o", "rays_d", "n_rays", "slots_per_ray", "xyz_min", "xyz_max", "near", "far", "stepdist") + MASK + (
    "act_shift", "interval", "thres") + OUT8 + ("stream",)
DENSE = ("density_grid", "X", "Y", "Z")
TENSORF = ("xy_plane", "xz_plane", "yz_plane", "x_vec", "y_vec", "z_vec", "X", "Y", "Z", "R", "Rxy", "comp_last")
COMPACT = ("n_rays", "n_samples", "act_shift", "interval", "thres", "scratch_pts", "scratch_density", "scratch_step", "scratch_w", "scratch_T",
           "count", "offset_end", "count2", "offset_end2", "t_table", "pts1", "density1", "weights1", "T1", "pos2", "pts2", "density2", "alpha2",
           "weights2", "ray_id2", "step_id2", "t2")
PARAMS = {
    "ugrid_train_march": FOURIER + ("scratch_pts", "scratch_density", "scratch_step", "count", "stream"),
    "ugrid_train_sample": FOURIER + OUT8 + ("stream",),
    "ugrid_train_sample_dcvgo": DENSE + DCVGO,
    "ugrid_train_sample_dvgo": DENSE + DVGO,
    "ugrid_train_sample_dcvgo_tensorf": TENSORF + DCVGO,
    "ugrid_train_sample_dvgo_tensorf": TENSORF + DVGO,
    "ugrid_train_sample_mpi": DENSE + ("rays_o", "rays_d", "n_rays", "n_steps", "xyz_min", "xyz_max", "act_shift", "mpi_depth") + MASK + (
        "interval", "thres") + OUT8 + ("stream",),
    "ugrid_train_sample_compact": COMPACT + ("stream",),
    "ugrid_train_sample_compact_vox": COMPACT + ("inner2", "stream"),
    "ugrid_train_sample_backward": ("n_rays", "act_shift", "interval", "density1", "weights1", "T1", "pos2", "count", "offset_end",
                                    "alphainv_last", "g_weights2", "g_alphainv_last", "g_density2", "g_density1", "stream"),
    "ugrid_train_compact": ("n_rays", "n_samples", "scratch_pts", "scratch_density", "scratch_step", "count", "offset_end", "t_table", "pts",
                            "density", "ray_id", "step_id", "t", "stream"),
}
MARCHES = ("ugrid_train_march", "ugrid_train_sample", "ugrid_train_sample_dcvgo", "ugrid_train_sample_dvgo", "ugrid_train_sample_dcvgo_tensorf",
           "ugrid_train_sample_dvgo_tensorf", "ugrid_train_sample_mpi")
# a well-formed call of one ray: what every case below spoils in ONE place
GOOD = {"n_rays": 1, "P": 5, "freq_num": 2, "X": 5, "Y": 7, "Z": 9, "R": 3, "Rxy": 2, "comp_last": 0, "n_samples": 8, "slots_per_ray": 8,
        "n_steps": 8, "mpi_depth": 4, "bg_len": 0.2, "norm_l2": 0, "dist_thres": 0.1, "near": 0.2, "far": 1e9, "stepdist": 0.1,
        "interval": 0.5, "thres": 1e-4, "stream": None}


@pytest.fixture(scope="module")
def lib():
    from unboundednerfpytorch_amd import _lib
    L = _lib.load()
    for name, params in PARAMS.items():
        assert len(params) == len(_lib._SIGNATURES[name][1]), name          # the name lists above follow the bound signatures
    return L


def _call(L, name, **spoil):
    from unboundednerfpytorch_amd import _lib
    args = []
    for p, ctype in zip(PARAMS[name], _lib._SIGNATURES[name][1]):
        if p in spoil:
            args.append(spoil[p])
        elif p in GOOD:
            args.append(GOOD[p])
        elif ctype is ctypes.c_void_p:
            args.append(PTR)
        else:
            args.append(0.0)      # act_shift as a number
    return getattr(L, name)(*args)


def _null_call(L, name, n_rays, **keep):
    from unboundednerfpytorch_amd import _lib
    args = [keep.get(p, n_rays if p == "n_rays" else (None if ctype is ctypes.c_void_p else 0))
            for p, ctype in zip(PARAMS[name], _lib._SIGNATURES[name][1])]
    return getattr(L, name)(*args)


@pytest.mark.parametrize("name", [n for n in PARAMS if not n.endswith("_tensorf")])
@pytest.mark.parametrize("n_rays", [0, -1])
def test_no_rays_is_no_work_whatever_else_is_passed(lib, name, n_rays):
    if name == "ugrid_train_sample":          # its stage-2 outputs come first (module docstring)
        assert _null_call(lib, name, n_rays) == 1
        assert _null_call(lib, name, n_rays, **{p: PTR for p in STAGE2}) == 0
        for p in STAGE2:
            assert _null_call(lib, name, n_rays, **{q: PTR for q in STAGE2 if q != p}) == 1, p
    else:
        assert _null_call(lib, name, n_rays) == 0


@pytest.mark.parametrize("name", ["ugrid_train_sample_dcvgo_tensorf", "ugrid_train_sample_dvgo_tensorf"])
def test_tensorf_marches_look_at_the_factors_before_the_ray_count(lib, name):
    factors = {p: PTR for p in TENSORF[:6]}
    dims = {"X": 5, "Y": 7, "Z": 9, "R": 3, "Rxy": 2}
    for n_rays in (0, -1):
        assert _null_call(lib, name, n_rays) == 1
        assert _null_call(lib, name, n_rays, **factors, **dims) == 0
    assert _call(lib, name, xy_plane=None) == 1 and _call(lib, name, R=0) == 1 and _call(lib, name, n_rays=0, z_vec=None) == 1


@pytest.mark.parametrize("name", MARCHES[1:])
@pytest.mark.parametrize("missing", STAGE2)
def test_a_missing_stage2_output_is_refused(lib, name, missing):
    assert _call(lib, name, **{missing: None}) == 1


@pytest.mark.parametrize("name", MARCHES)
def test_sample_counts_must_be_positive(lib, name):
    slots = "n_steps" if name.endswith("_mpi") else "slots_per_ray" if "_dvgo" in name else "n_samples"
    for n in (0, -1):
        assert _call(lib, name, **{slots: n}) == 1, n
    if name.endswith("_mpi"):                 # j / (n_steps - 1): at least two samples
        assert _call(lib, name, n_steps=1) == 1


@pytest.mark.parametrize("name", ["ugrid_train_march", "ugrid_train_sample"])
def test_level_count_must_match_the_frequency_count(lib, name):
    for P, freq_num in ((3, 2), (6, 2), (2, 0), (0, 0), (1, 1)):
        assert _call(lib, name, P=P, freq_num=freq_num) == 1, (P, freq_num)


@pytest.mark.parametrize("name", ["ugrid_train_sample_dvgo", "ugrid_train_sample_dvgo_tensorf"])
def test_dvgo_step_length_must_be_positive(lib, name):
    for stepdist in (0.0, -0.1, float("nan")):
        assert _call(lib, name, stepdist=stepdist) == 1, stepdist


@pytest.mark.parametrize("name", ["ugrid_train_sample_dcvgo", "ugrid_train_sample_dcvgo_tensorf"])
def test_dcvgo_needs_its_t_table(lib, name):
    assert _call(lib, name, t_table=None) == 1


def test_mpi_limits(lib):
    for depth in (0, -1, 257):
        assert _call(lib, "ugrid_train_sample_mpi", mpi_depth=depth) == 1, depth
    assert _call(lib, "ugrid_train_sample_mpi", act_shift=None) == 1


@pytest.mark.parametrize("name", MARCHES[2:])
def test_mask_cache_arguments(lib, name):
    assert _call(lib, name, mask_dims3=None) == 1
    dims = (ctypes.c_int32 * 3)(2, 3, 4)      # read by the entry point: a real array
    where = ctypes.cast(dims, ctypes.c_void_p).value
    for null in ("mask", "xyz2ijk_scale3", "xyz2ijk_shift3"):
        assert _call(lib, name, mask_dims3=where, **{null: None}) == 1, null
    for k in range(3):
        bad = (ctypes.c_int32 * 3)(2, 3, 4)
        bad[k] = 0
        assert _call(lib, name, mask_dims3=ctypes.cast(bad, ctypes.c_void_p).value) == 1, k
