"""Drop-in `dataloaders` package: `test_dataset` and `inpainting_dataset` are replaced (`raw_pairs` is this package's own);
`inpainting_crossview_dataset` and `obj_nvs_dataset` are provided where no other tree brings its own.

The reference's `dataloaders` is a namespace directory that also holds inpainting_crossview_dataset and
obj_nvs_dataset (training / multi-view entry points import them).  A regular package would shadow those, so this package
appends every other `dataloaders` directory found on sys.path to its search path: `dataloaders.test_dataset` and `dataloaders.inpainting_dataset` resolve here,
everything else still resolves to the reference's files.  `dataloaders.inpainting_crossview_dataset` and `dataloaders.obj_nvs_dataset` resolve to this build's modules
only when none of those directories holds one (the modules step aside themselves); this build's tools import them as
`leftrefill_amd.dropin.dataloaders.inpainting_crossview_dataset` / `.obj_nvs_dataset`, which are always this build's.
"""
import os
import sys

_here = os.path.dirname(os.path.abspath(__file__))
for _p in list(sys.path):
    _d = os.path.join(_p or os.getcwd(), "dataloaders")
    if os.path.isdir(_d) and os.path.abspath(_d) != _here and _d not in __path__:
        __path__.append(_d)
