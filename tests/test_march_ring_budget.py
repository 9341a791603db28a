"""Build-quality guard for k_march_ring<F, L2, W> (no GPU needed): the ring kernels keep everything in registers -- no VGPR / SGPR
spills, no scratch (a scratch access inside the ring would be a vector-memory operation the hand-placed vmcnt waits do not count) --
and stay inside the register cap of the waves per SIMD they are built for: 512 / 7 -> 72 at W = 7, 64 at W = 8.  All 20 instantiations
(F = 1..5 x both contractions x W = 7, 8) must be in the library: a missing kernel is an error, not a fall-back."""
import os
import re

from test_capi import ROOT, _kernel_metadata


def test_march_ring_kernels_fit_their_register_cap_without_scratch():
    meta = _kernel_metadata(os.path.join(ROOT, "unboundednerfpytorch_amd", "libugrid_hip.so"))
    found = {}
    for k, m in meta.items():
        w = re.match(r"_Z12k_march_ringILi(\d)ELb([01])ELi(\d)EE", k)
        if not w:
            continue
        F, l2, W = int(w.group(1)), int(w.group(2)), int(w.group(3))
        found[(F, l2, W)] = m
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, (k, m)
        assert m["vgpr_count"] <= {7: 72, 8: 64}[W], (k, m)
    assert sorted(found) == sorted((F, l2, W) for F in range(1, 6) for l2 in (0, 1) for W in (7, 8)), sorted(found)
    # the plain kernels stop at 6 waves: 7 and 8 are the ring kernels only
    assert not [k for k in meta if re.match(r"_Z7k_marchILi\dELb[01]ELi[789]EE", k)]
