"""What the makers of the dataset goldens (make_golden_pair_datasets.py, make_golden_nvs_dataset.py) share: constructor keywords with
"@name" paths, a seeded sequence of items, the import of a reference module by path behind a stand-in `cv2`, and the tally of the
reference branches a run takes.  The stand-ins, trees and item packings are each maker's own."""
import contextlib
import importlib.util
import os
import random
import sys

import numpy as np


def resolve(kwargs, root):
    """Constructor keywords with "@name" entries (also inside lists) turned into paths under root."""
    at = lambda v: os.path.join(root, v[1:]) if isinstance(v, str) and v.startswith("@") else v
    return {k: [at(x) for x in v] if isinstance(v, list) else at(v) for k, v in kwargs.items()}


def run_sequence(cls, kwargs, seed, indices, root, **extra):
    """Seed both generators, build `cls(**kwargs, **extra)`, take the items in order; (items, next random.random(), next
    np.random.random())."""
    ds = cls(**resolve(kwargs, root), **extra)
    random.seed(seed)
    np.random.seed(seed)
    items = [ds[i] for i in indices]
    return items, random.random(), np.random.random()


def import_reference(ref_dir, module, cv2):
    """The reference checkout's dataloaders/<module>.py, executed from its file with `cv2` standing in for OpenCV: (module, its path)."""
    path = os.path.join(ref_dir, "dataloaders", module + ".py")
    sys.modules["cv2"] = cv2
    spec = importlib.util.spec_from_file_location("reference_" + module, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, path


@contextlib.contextmanager
def branch_tally(ref_file, branch_lines):
    """While the block runs, count the executions of `ref_file`'s lines named in `branch_lines` (line -> branch name); yields the
    tally {branch name: count}."""
    tally = {name: 0 for name in branch_lines.values()}

    def tracer(frame, event, arg):
        if frame.f_code.co_filename != ref_file:
            return None
        if event == "line" and frame.f_lineno in branch_lines:
            tally[branch_lines[frame.f_lineno]] += 1
        return tracer

    sys.settrace(tracer)
    try:
        yield tally
    finally:
        sys.settrace(None)
