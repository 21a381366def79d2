import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    import oraclelib
    return oraclelib.Oracle()


@pytest.fixture(scope="session")
def ref():
    """The compiled reference where oracle/_ref is built, else its answers recorded under tests/golden/
    (oraclelib.open_ref)."""
    import oraclelib
    r = oraclelib.open_ref()
    yield r
    if isinstance(r, oraclelib.RecordedRef) and r.live is not None:
        r.save()


@pytest.fixture(scope="session")
def decoder():
    import oraclelib
    return oraclelib.Decoder()
