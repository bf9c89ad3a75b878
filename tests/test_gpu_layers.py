"""GPU: every replica layer x every flavour x every input form. A replica answers through the super-k-mer table (the default),
or -- every shard of a minimizer-sharded index, a table that does not fit, SSHASH_AMD_SKTABLE=0 -- through the minimizer directory
or the MPHF alone (device_layout.hpp (3)-(5)), and each layer runs kernel instances of its own: without the table the first pass
hands MIDLOAD buckets to the bucket-scan pass, the streaming query runs its table-less state machine and the streaming lookup the
masked multi-pass kernels. The layer is read when a replica is uploaded, so each one runs in a process of its own
(tests/gpu_layer_worker.py), one after the other: k from 15 to 63 (one and two words, every word of the ASCII packer), regular and
canonical, packed and ASCII input from host and device buffers at aligned and unaligned addresses, neighbours and streaming, every
field against the CPU oracle."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from gpu_layer_worker import DICTIONARIES, LAYERS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layer", list(LAYERS))
def test_every_flavour_and_input_form_on_the_layer(layer):
    env = dict(os.environ)
    for switch in ("SSHASH_AMD_SKTABLE", "SSHASH_AMD_DIRECTORY", "SSHASH_AMD_TEST_HOOKS"):
        env.pop(switch, None)
    env.update(LAYERS[layer][0])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_layer_worker.py"), layer], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["ok"] and got["layer"] == layer
    assert len(got["dictionaries"]) == len(DICTIONARIES) + 1
    for name, st in got["dictionaries"].items():
        if name != "single_kmer":
            assert (st["sk_slots"] > 0) == (layer == "table"), (name, st)
