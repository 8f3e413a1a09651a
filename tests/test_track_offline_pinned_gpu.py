"""GPU: the BYTES of the whole-recording track read-outs - sf_track_decode, sf_track_posterior, sf_track_pairwise and their gated forms behind ops.track_decode /
track_posterior / track_pairwise / track_decode_gated / track_posterior_gated / track_pairwise_gated - held to the SHA-256 recorded once from the tree and the library of
the commit that tests/golden/track_offline_digests.json names.

The oracle files (test_track_gpu.py, test_track_posterior_gpu.py, test_track_gated_gpu.py, test_track_pairwise_gpu.py) judge a path by its score and the marginals
within a bar: they pass a changed order of a sum or a multiply-add that was two operations.  The plain and the gated read-out share their scans, combine, backtrace and launchers as templates over two
chains (csrc/sf_track.hip), so a change to a shared body moves both; this file is what shows whether it moved a bit.  A case digests every tensor the three calls return, in
order; tests/golden/make_track_offline_digests.py lists the cases (chain x C x W at the sizes where a kernel takes another path, plus a masked class, strided inputs and
pairwise without xi) and says how the file is recorded.  The input's own digest is checked first: a mismatch there is a changed random stream, not a changed kernel.
54 cases of at most 257 rows: about 1 s on an MI355X."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_track_offline_digests as TD  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def digests():
    with open(TD.OUT) as f:
        return json.load(f)['cases']


def test_the_recording_has_the_generators_cases(digests):
    assert set(digests) == set(TD.CASES)


@pytest.mark.parametrize('name', list(TD.CASES))
def test_track_offline_outputs_are_pinned(gpu, digests, name):
    assert TD.input_digest(name) == digests[name]['input'], f'{name}: the generated INPUT differs from the recorded one'
    assert TD.CASES[name].run(gpu) == digests[name]['output'], f'{name}: output bytes differ from the recording'
