"""CPU: every prototype and struct of include/leftrefill_hip.h against its ctypes mirror in leftrefill_amd/_lib.py (tests/abi_helpers.py).
A wrong kind in the mirror (c_int for an int64_t, a float one slot off) hands a kernel a garbage pointer: a GPU fault, not an exception."""
import ctypes

import numpy as np

import abi_helpers as abi
from leftrefill_amd import _lib, dataprep, nvsprep, refill


def test_symbols_match_header():
    h = abi.header()
    assert len(h.protos) >= 120 and len(h.structs) == 15 and set(h.dev_protos) >= {"lr_dev_set", "lr_dev_unset"}
    assert set(h.protos) == set(_lib.SIGNATURES) and set(h.dev_protos) == set(_lib.DEV_SIGNATURES)


def test_every_signature_matches_header():
    assert abi.check_signatures({**_lib.SIGNATURES, **_lib.DEV_SIGNATURES}, _lib.INT64_RETURNS, _lib.STRUCTS) == []


def test_bf16_twins_match_their_fp16_forms():
    assert abi.check_twins(_lib.BF16_TWINS, _lib.twin) == [] and len(set(_lib.BF16_TWINS)) == len(_lib.BF16_TWINS)


def test_every_struct_matches_header_and_compiler():
    mirrors = {c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}
    assert mirrors == set(_lib.STRUCTS.values()), "a Structure of _lib.py is missing from _lib.STRUCTS"
    assert abi.check_structs(_lib.STRUCTS) == []


def test_job_dtypes_are_the_mirrors():
    for mod, mirror in ((dataprep, _lib.PrepJob), (nvsprep, _lib.NvsJob), (refill, _lib.PilJob)):
        assert mod.JOB_DTYPE == np.dtype(mirror), mod.__name__


# ---- the checker rejects broken mirrors (doctored copies; the real tables are never edited) -----------------------------------------
def test_checker_rejects_a_widened_int():
    args = list(_lib.SIGNATURES["lr_layernorm"])
    i = args.index(_lib.c_int)
    args[i] = _lib.c_int64
    bad = abi.check_signatures({**_lib.SIGNATURES, "lr_layernorm": args}, _lib.INT64_RETURNS, _lib.STRUCTS)
    assert len(bad) == 1 and bad[0].startswith(f"lr_layernorm #{i}:"), bad


def test_checker_rejects_swapped_fields():
    fields = list(_lib.LoraDrop._fields_)
    fields[0], fields[1] = fields[1], fields[0]
    bad = abi.check_structs({**_lib.STRUCTS, "lr_lora_drop": type("Swapped", (ctypes.Structure,), {"_fields_": fields})})
    assert bad[0].startswith("lr_lora_drop: fields") and "lr_lora_drop.seed: (8, 8) != (0, 8)" in bad, bad


def test_checker_rejects_a_dropped_twin():
    bad = abi.check_twins([n for n in _lib.BF16_TWINS if n != "lr_rowlin_f16"], _lib.twin)
    assert len(bad) == 1 and "lr_rowlin_bf16" in bad[0], bad
