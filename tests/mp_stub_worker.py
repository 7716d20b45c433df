"""One rank of tests/test_mp_launch.py: no GPU, no ga_amd, no torch -- it stands in for a GA worker.

It touches $STUB_STARTED.<rank> first (where STUB_STARTED is set), prints the environment the
launcher gave it as "ENV <name>=<value>" lines and $STUB_SAY, and then, by mode:
  ok      prints "RANK <r> OK"
  fail    exits with status 5
  hang    rank 0 sleeps far past any limit of the tests; the other ranks end as in ok
  abort   prints "ABORT EXPECTED" and "stub: the message", exits with status 1
"""
import os
import sys
import time

rank = os.environ["RANK"]
if os.environ.get("STUB_STARTED"):
    open(f"{os.environ['STUB_STARTED']}.{rank}", "w").close()
for name in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "COMEX_AMD_JOBID",
             "COMEX_AMD_STAGING_MB", "TEST_STACK_DUMP_S"):
    print(f"ENV {name}={os.environ[name]}")
print(f"ARGS {sys.argv[1:]}")
if os.environ.get("STUB_SAY"):
    print(os.environ["STUB_SAY"])
sys.stdout.flush()
mode = sys.argv[1] if len(sys.argv) > 1 else "ok"
if mode == "fail":
    sys.exit(5)
if mode == "hang" and rank == "0":
    time.sleep(600)
if mode == "abort":
    print("ABORT EXPECTED\nstub: the message", flush=True)
    sys.exit(1)
print(f"RANK {rank} OK", flush=True)
