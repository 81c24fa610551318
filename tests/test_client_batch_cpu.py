"""CPU: the batched client calls on the host path (EVA_DEVICE_CLIENT=0), the part that needs no GPU.
secret_ctx.encrypt_batch's stream contract (one pair of streams per call, instances in list order, names sorted within an
instance, 4 seed words + one sample_error per encrypted input), decrypt_batch == a loop of decrypt (float64 bit patterns),
the input checks with encrypt()'s messages, and an encrypt_batch -> decrypt_batch round trip within the reference's
statistical oracle (MSE < 0.01, as tests/test_host_e2e_cpu.py)."""
import numpy as np
import pytest

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.metric import valuation_mse
from eva.seal import generate_keys


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def _program(vec=64, N=2048, plain=False):
    prog = EvaProgram('batch', vec_size=vec)
    with prog:
        x, y, w = Input('x'), Input('y'), Input('w', not plain)
        Output('z', x * y + w)
        Output('d', x - y)
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


def _inputs(B, vec=64, seed=1):
    rng = np.random.default_rng(seed)
    return [{n: list(rng.uniform(-2, 2, vec)) for n in ('x', 'y', 'w')} for _ in range(B)]


def _same(a, b):
    assert sorted(a.names()) == sorted(b.names())
    for n in a.names():
        x, y = a.get(n), b.get(n)
        assert x[:4] == y[:4], (n, x[:4], y[:4])
        assert np.array_equal(np.asarray(x[4]), np.asarray(y[4])), f"value {n} differs"


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def test_secret_encrypt_batch_stream_contract():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 3)
    xs = _inputs(3)
    encs = sec.encrypt_batch(xs, sig, seed=7)
    assert len(encs) == 3
    # a batch of one is encrypt() word for word, and so is instance 0 of a longer batch
    _same(sec.encrypt_batch(xs[:1], sig, seed=7)[0], sec.encrypt(xs[0], sig, seed=7))
    _same(encs[0], sec.encrypt(xs[0], sig, seed=7))
    # no two encrypted values of the call share a seed
    seeds = [e.seed(n) for e in encs for n in ('w', 'x', 'y')]
    assert all(s is not None and len(s) == 32 for s in seeds) and len(set(seeds)) == 9
    # names are visited sorted within an instance whatever the dict's order, instances in list order: the seeds are the
    # consecutive 32-byte pieces of one stream.  encrypt() of {'w'} alone takes the first piece, of {'w', 'x'} the first two.
    shuffled = [{n: x[n] for n in ('y', 'w', 'x')} for x in xs]
    again = sec.encrypt_batch(shuffled, sig, seed=7)
    for a, b in zip(encs, again):
        _same(a, b)
    assert encs[0].seed('w') == sec.encrypt_batch([xs[1]], sig, seed=7)[0].seed('w')  # first draw of the stream, whatever the data
    # instance 1's values differ from encrypt(xs[1], seed=7): it continues the call's streams instead of restarting them
    assert encs[1].seed('w') != sec.encrypt(xs[1], sig, seed=7).seed('w')
    # every value decrypts to its input
    for x, e in zip(xs, encs):
        got = sec.decrypt(e, sig)
        for n in x:
            assert np.abs(np.array(got[n]) - np.array(x[n])).max() < 1e-4


def test_secret_encrypt_batch_plain_and_raw_inputs():
    compiled, params, sig = _program(plain=True)
    pub, sec = generate_keys(params, 3)
    xs = _inputs(2)
    encs = sec.encrypt_batch(xs, sig, seed=5)
    for b in range(2):
        assert encs[b].seed('w') is None and encs[b].seed('x') is not None
    _same(encs[0], sec.encrypt(xs[0], sig, seed=5))
    # only encrypted inputs take draws: x and y of instance 0, then x and y of instance 1
    assert len({encs[b].seed(n) for b in range(2) for n in ('x', 'y')}) == 4


def test_public_encrypt_batch_and_round_trip():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 4)
    xs = _inputs(5, seed=2)
    for encs in (pub.encrypt_batch(xs, sig), sec.encrypt_batch(xs, sig)):
        assert len(encs) == 5
        outs = sec.decrypt_batch(encs, sig)
        assert len(outs) == 5
        for x, o in zip(xs, outs):
            assert sorted(o) == ['w', 'x', 'y']
            assert valuation_mse(o, x) < 0.01
    assert pub.encrypt_batch([], sig) == [] and sec.encrypt_batch([], sig) == [] and sec.decrypt_batch([], sig) == []


def test_decrypt_batch_equals_a_loop_of_decrypt():
    compiled, params, sig = _program(plain=True)
    pub, sec = generate_keys(params, 6)
    xs = _inputs(4, seed=3)
    encs = sec.encrypt_batch(xs, sig, seed=9)[:2] + [pub.encrypt(x, sig) for x in xs[2:]]
    outs = sec.decrypt_batch(encs, sig)
    for e, o in zip(encs, outs):
        want = sec.decrypt(e, sig)
        assert sorted(o) == sorted(want)
        for n in want:
            assert np.array_equal(_bits(o[n]), _bits(want[n])), f"output {n}"


def test_encrypt_batch_input_checks():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 8)
    xs = _inputs(3)

    def message(call, arg):
        with pytest.raises(Exception) as e:
            call(arg, sig)
        return str(e.value)

    for ctx in (pub, sec):
        short = [dict(x) for x in xs]
        short[2]['x'] = short[2]['x'][:-1]
        assert message(ctx.encrypt_batch, short) == message(ctx.encrypt, short[2]) == "Input size does not match program vector size"
        extra = [dict(x, q=x['x']) for x in xs]
        assert message(ctx.encrypt_batch, extra) == message(ctx.encrypt, extra[0])
        assert "No input named q" in message(ctx.encrypt_batch, extra)
        # every instance names the inputs of instance 0
        missing = [dict(x) for x in xs]
        del missing[1]['y']
        assert "instance 1" in message(ctx.encrypt_batch, missing)
        renamed = [dict(x) for x in xs]
        renamed[2]['q'] = renamed[2].pop('y')
        assert "instance 2" in message(ctx.encrypt_batch, renamed)
    # a signature whose vector size does not fit the slots: encrypt()'s message
    compiled2, params2, sig2 = _program(vec=4096, N=2048)
    big = [{n: [0.5] * 4096 for n in ('x', 'y', 'w')}]
    for ctx in (pub, sec):
        with pytest.raises(Exception) as e1:
            ctx.encrypt_batch(big, sig2)
        with pytest.raises(Exception) as e2:
            ctx.encrypt(big[0], sig2)
        assert str(e1.value) == str(e2.value) == "Vector size cannot be larger than slot count"


def test_decrypt_batch_refuses_none_by_index():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 4)
    encs = sec.encrypt_batch(_inputs(2), sig, seed=2)
    with pytest.raises(ValueError, match="valuation 1 is None"):
        sec.decrypt_batch([encs[0], None, encs[1]], sig)
