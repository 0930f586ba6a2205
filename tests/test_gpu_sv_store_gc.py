"""The drivers' store and dead caches (orca_amd/sv.py, `GenomeEncodings._s3_make`): a store that was dropped is cyclic garbage - its
ChromEncodings reach it back through their `codes` callables - so the HBM of its stage caches is held until Python's cycle collector runs.
Before a new cache is given up for lack of HBM the collector is run.  Shown with the collector switched off and a memory figure that says
"none" for as long as the dead cache is alive; no sizes of the machine enter."""
import gc
import weakref

import pytest

from orca_amd import orca_models, sv, sv_drivers, synth

pytestmark = pytest.mark.gpu


def test_a_dropped_stores_cache_is_collected_before_a_new_one_is_given_up(cuda, monkeypatch):
    model = orca_models.H1esc(synthetic_seed=0)
    g = synth.sv_driver_genome().to(cuda)
    piece = [("chrS", 10_000_000, 2_000_000, "+")]                           # the cached region: +- 4 Mb around it, 10 GB
    sv_drivers.clear_encoding_cache()
    gc.collect()
    gc.disable()
    try:
        store = sv_drivers._store(g, model.net0)
        store.s3_after = 1
        old = store.stage3_caches(piece, True)["chrS"]
        assert len(old.entries) == 160
        dead = weakref.ref(old)
        del old, store
        sv_drivers.clear_encoding_cache()
        assert dead() is not None                                            # reference counts alone do not free it
        real = sv._hbm_available
        monkeypatch.setattr(sv, "_hbm_available", lambda dev: real(dev) if dead() is None else 0.0)
        store = sv_drivers._store(g, model.net0)
        store.s3_after = 1
        new = store.stage3_caches(piece, True)
        assert dead() is None and len(new["chrS"].entries) == 160
    finally:
        gc.enable()
        sv_drivers.clear_encoding_cache()
