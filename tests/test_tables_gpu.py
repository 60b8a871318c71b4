"""The model tables as haf_create leaves them on the device, against the digests recorded from the commit before the table work was
split into model_tables.cpp and upload_tables (tests/golden/table_digests.json, tests/golden/make_table_digests.py): every device
table byte for byte, every member of every parameter struct, every scalar and flag.  Creations only, no request."""
import pytest

import table_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return table_cases.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("table_models")


@pytest.mark.parametrize("name", sorted(table_cases.CASES))
def test_device_tables_match_recorded_digests(name, fixture, data_dir, golden_dir, model_dir):
    want = fixture["cases"][name]
    got = table_cases.device_digests(name, data_dir, golden_dir, model_dir)
    assert sorted(got) == sorted(want)
    moved = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not moved, moved
