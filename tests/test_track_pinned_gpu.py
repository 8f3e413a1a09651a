"""GPU: the BYTES of the fixed-lag read-outs of live feeds - sf_track_stream_push, sf_track_pool_push and their gated forms behind ops.track_stream_push /
track_pool_push / track_stream_push_gated / track_pool_push_gated - held to the SHA-256 recorded once from the tree and the library of the commit that
tests/golden/track_stream_digests.json names.

The oracle files (test_track_stream_gpu.py, test_track_pool_gpu.py, test_track_gated_stream_gpu.py) judge a path by its score and the posterior within a bar: they pass a
changed order of a sum, a multiply-add that was two operations, a state byte that moved.  The plain and the gated read-out are one set of templates over two chains
(csrc/sf_track.hip), so a change to the shared bodies moves both; this file is what shows whether it moved a bit.  A case digests every tensor of every push's result in
field order and the state buffer after every push; tests/golden/make_track_stream_digests.py lists the cases (stream: C x lag x posterior x two ways to close, through one
chunk pattern, plus a masked class and strided inputs; pool: 5 slots over 4 ragged ticks) and says how the file is recorded.  The input's own digest is checked first: a
mismatch there is a changed random stream, not a changed kernel.  128 cases of a few hundred rows: about 2 s on an MI355X."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_track_stream_digests as TD  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def digests():
    with open(TD.OUT) as f:
        return json.load(f)['cases']


def test_the_recording_has_the_generators_cases(digests):
    assert set(digests) == set(TD.CASES)


@pytest.mark.parametrize('name', list(TD.CASES))
def test_track_stream_outputs_are_pinned(gpu, digests, name):
    assert TD.input_digest(name) == digests[name]['input'], f'{name}: the generated INPUT differs from the recorded one'
    assert TD.CASES[name].run(gpu) == digests[name]['output'], f'{name}: output or state bytes differ from the recording'
