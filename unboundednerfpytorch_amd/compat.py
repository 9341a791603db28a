"""Register this package's modules under the names the reference imports at module top
(`import render_utils_cuda`, `import total_variation_cuda`, `import ub360_utils_cuda`,
`import adam_upd_cuda` -- dvgo.py:13, grid.py:10-11, FourierGrid_grid.py:10-11, dcvgo.py:15,
FourierGrid_model.py:17-18, masked_adam.py:3), so run_train.py / run_render.py / MaskedAdam of the
reference call the MI355X kernels unchanged.  Call before importing any reference model file."""
import sys


def install_as_reference_extensions(native=False):
    """native=False: the ctypes mirrors of this package (always available).  native=True: the pybind11 modules of binding/
    (what a maintainer would build in place of FourierGrid/cuda/*.cu; `python binding/build.py`)."""
    if native:
        import os
        import sys as _sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if root not in _sys.path:
            _sys.path.insert(0, root)
        from binding import build as _b
        if not _b.available():
            raise RuntimeError("binding/_build is empty: run `python binding/build.py` (needs torch headers and libugrid_hip.so)")
        return tuple(_b.install())
    from . import adam_upd_cuda, render_utils_cuda, total_variation_cuda, ub360_utils_cuda
    for mod in (render_utils_cuda, total_variation_cuda, ub360_utils_cuda, adam_upd_cuda):
        sys.modules[mod.__name__.rsplit(".", 1)[-1]] = mod
    return ("render_utils_cuda", "total_variation_cuda", "ub360_utils_cuda", "adam_upd_cuda")


def install_model_classes(package="FourierGrid"):
    """Rebind the reference's three model classes to this package's training models -- `<package>.dvgo.DirectVoxGO`,
    `<package>.dcvgo.DirectContractedVoxGO`, `<package>.FourierGrid_model.FourierGridModel` -- so that the reference's training
    program builds them (run_train.py:19-56 create_new_model), dispatches on them (`isinstance` at :191-196, :380) and checkpoints
    them unchanged, with the fused training forwards of this package underneath.  Call after install_as_reference_extensions(),
    with the reference tree on sys.path, BEFORE importing `<package>.run_train` (which binds FourierGridModel by name at import,
    run_train.py:10).  Returns the three original classes (to restore them: setattr them back)."""
    import importlib
    from . import fourier_model, voxgo_model
    dv = importlib.import_module(package + ".dvgo")
    dc = importlib.import_module(package + ".dcvgo")
    fg = importlib.import_module(package + ".FourierGrid_model")
    orig = (dv.DirectVoxGO, dc.DirectContractedVoxGO, fg.FourierGridModel)
    dv.DirectVoxGO = voxgo_model.DirectVoxGO
    dc.DirectContractedVoxGO = voxgo_model.DirectContractedVoxGO
    fg.FourierGridModel = fourier_model.FourierGridModel
    rt = sys.modules.get(package + ".run_train")
    if rt is not None and hasattr(rt, "FourierGridModel"):       # already imported: rebind its by-name import too
        rt.FourierGridModel = fourier_model.FourierGridModel
    return orig


def install_mpi_model_class(package="FourierGrid"):
    """Rebind `<package>.dmpigo.DirectMPIGO` -- the model create_new_model builds for forward-facing scenes (cfg.data.ndc,
    run_train.py:19-56) and run_train.py:190 dispatches on -- to mpi_model.DirectMPIGO, as install_model_classes does for the other
    three.  Same calling order (after install_as_reference_extensions(), the reference tree on sys.path); a `<package>.run_train`
    that is already imported has its module reference `dmpigo` in common, so nothing else needs rebinding.  Returns the original
    class (to restore it: setattr it back)."""
    import importlib
    from . import mpi_model
    dm = importlib.import_module(package + ".dmpigo")
    orig = dm.DirectMPIGO
    dm.DirectMPIGO = mpi_model.DirectMPIGO
    return orig


def install_metrics(utils_module):
    """Set `utils_module.rgb_ssim` (the reference's FourierGrid.utils, or any module object with that attribute) to this package's
    metrics.rgb_ssim -- same positional signature, evaluated by the HIP kernel -- so that the reference's own
    run_render.render_viewpoints(..., eval_ssim=True) (run_render.py:77-78 calls utils.rgb_ssim(rgb, gt, max_val=1)) scores its
    frames on the GPU.  Returns the function it replaced (setattr it back to restore)."""
    from . import metrics
    orig = getattr(utils_module, "rgb_ssim", None)
    utils_module.rgb_ssim = metrics.rgb_ssim
    return orig
