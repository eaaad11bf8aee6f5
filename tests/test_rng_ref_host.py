"""tests/rng_ref.py against the sources: its table of Philox tags is the list of #define CRL_TAG_* lines of crl_common.hpp."""
import os
import re

from tests import rng_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tags_are_those_of_crl_common():
    with open(os.path.join(ROOT, "colosseumrl_amd", "csrc", "crl_common.hpp")) as f:
        defined = re.findall(r"^#define\s+(CRL_TAG_\w+)\s+(0x[0-9a-fA-F]+)u", f.read(), re.M)
    assert len(defined) == 12 and {name: int(value, 16) for name, value in defined} == rng_ref.TAGS
    assert len(set(rng_ref.TAGS.values())) == 12
    for name, value in rng_ref.TAGS.items():
        assert getattr(rng_ref, name, value) == value and rng_ref.tag_hex(name).lower() == "0x%08x" % value
