"""Records tests/golden/table_digests.json on an MI355X: the digests of every model table, parameter struct and scalar that haf_create's
table work leaves in the engines of tests/table_cases.py (haf_test_table_digest of the testing library).

Run it on the commit whose tables are the reference -- never on the code under test:  python tests/golden/make_table_digests.py [OUT.json]
"""
import json
import os
import platform
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import table_cases  # noqa: E402


def compiler_version():
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    out = subprocess.check_output([hipcc, "--version"]).decode(errors="replace")
    return [ln.strip() for ln in out.splitlines() if "version" in ln]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, table_cases.FIXTURE)
    data = os.path.join(HERE, "data")
    rec = {"libc": list(platform.libc_ver()), "compiler": compiler_version(), "env": table_cases.BASE_ENV, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(table_cases.CASES):
            rec["cases"][name] = table_cases.device_digests(name, data, HERE, tmp)
            print(name, len(rec["cases"][name]), "digests", flush=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
