"""What tests/golden/make_golden_api.py asks the UNMODIFIED reference and tests/test_host_api.py asks the mirror: the
parameters and defaults of every name a user can reach, and the answers of ``_is_series_of_strings`` on every kind of
Series.  The reference's answers are recorded in tests/golden/reference_api.json."""
import inspect
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_api.json")


def surface(mod):
    """Module constants, top-level functions, StringGrouper's members incl. the private ones and StringGrouperConfig
    of a ``string_grouper.string_grouper`` module, as JSON-ready lists."""
    def params(o):
        return [[p.name, repr(p.default), str(p.kind)] for p in inspect.signature(o).parameters.values()]

    return {"consts": {n: repr(getattr(mod, n)) for n in dir(mod) if n.isupper()},
            "funcs": {n: params(o) for n, o in vars(mod).items() if inspect.isfunction(o) and o.__module__ == mod.__name__},
            "methods": {n: (params(o) if callable(o) else None)
                        for n, o in inspect.getmembers(mod.StringGrouper) if not (n.startswith("__") and n != "__init__")},
            "config": [list(mod.StringGrouperConfig._fields),
                       {k: repr(v) for k, v in mod.StringGrouperConfig._field_defaults.items()}]}


def series_cases():
    return {
        "object str": pd.Series(["a", "b"]), "string dtype": pd.Series(["a", "b"], dtype="string"),
        "arrow": pd.Series(["a", "b"], dtype="string[pyarrow]"), "categorical of str": pd.Series(["a", "b", "a"], dtype="category"),
        "categorical of int": pd.Series(pd.Categorical([1, 2])), "mixed": pd.Series(["a", 1]), "none": pd.Series(["a", None]),
        "nan": pd.Series(["a", np.nan]), "pd.NA in string dtype": pd.Series(["a", pd.NA], dtype="string"),
        "ints": pd.Series([1, 2]), "floats": pd.Series([1.0]), "bytes": pd.Series([b"a"]),
        "empty object": pd.Series([], dtype=object), "empty float": pd.Series([], dtype=float),
        "empty string": pd.Series([], dtype="string"), "empty category": pd.Series([], dtype="category"),
        "not a series": ["a", "b"], "frame": pd.DataFrame({"a": ["x"]}), "index": pd.Index(["a"]),
        "datetimes": pd.Series(pd.date_range("2020", periods=2)), "bools": pd.Series([True, False]),
    }


def ask(f, v):
    try:
        return bool(f(v))
    except Exception as e:           # (the reference's map/any chain raises on some extension dtypes: nothing to compare)
        return "raises " + type(e).__name__


def series_answers(string_grouper_cls):
    return {k: ask(string_grouper_cls._is_series_of_strings, v) for k, v in series_cases().items()}
