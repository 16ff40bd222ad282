"""CPU: every torch.autograd.Function of ltr_mi355x has an entry in the table of tests/test_autograd_state_gpu.py (what a backward
gets from its forward when the caller does something in between), and the table names nothing that is gone."""
import glob
import importlib
import inspect
import os

import torch


def _package_functions():
    import ltr_mi355x
    found = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(ltr_mi355x.__file__), "*.py"))):       # (the built .so files are no modules)
        mod = importlib.import_module(f"ltr_mi355x.{os.path.basename(path)[:-3]}")
        for name, obj in inspect.getmembers(mod, inspect.isclass):
            if issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__:
                found[name] = mod.__name__
    return found


def test_every_autograd_function_has_a_state_table_entry():
    from test_autograd_state_gpu import ENTRIES, FUNCTIONS
    found = _package_functions()
    assert len(found) >= 22, found
    assert set(FUNCTIONS) == set(found), ("missing from the table", sorted(set(found) - set(FUNCTIONS)),
                                          "not in the package", sorted(set(FUNCTIONS) - set(found)))
    assert len({e.name for e in ENTRIES}) == len(ENTRIES), "entry names must be unique (they are the test ids)"
