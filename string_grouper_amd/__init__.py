"""string_grouper_amd -- MI355X-native core for string_grouper's fuzzy-matching hot path.

Public surface = the reference's (string_grouper/__init__.py:1-2): the four module-level functions,
``StringGrouper`` and ``StringGrouperConfig`` -- plus ``Corpus``, a master list fitted once and kept on the device
(string_grouper_amd/corpus.py), ``pair_similarities``, the score of named row pairs (string_grouper_amd/pairs.py), and
``match_records``, matching on several fields (string_grouper_amd/records.py; the ``string_grouper`` alias keeps the
reference's surface).  The compute runs in libsg_hip.so (hand-written HIP
kernels for gfx950, C ABI in include/sg_hip.h); there is no CPU fallback."""
from .corpus import Corpus  # noqa: F401
from .pairs import pair_similarities  # noqa: F401
from .records import match_records  # noqa: F401
from .string_grouper import (StringGrouper, StringGrouperConfig, StringGrouperNotFitException,  # noqa: F401
                             compute_pairwise_similarities, group_similar_strings, match_most_similar,
                             match_strings)

__all__ = ["Corpus", "StringGrouper", "StringGrouperConfig", "StringGrouperNotFitException", "compute_pairwise_similarities",
           "group_similar_strings", "match_most_similar", "match_records", "match_strings", "pair_similarities"]
