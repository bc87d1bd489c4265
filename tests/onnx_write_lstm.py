"""Write a recurrent actor (a Policy with an LSTM) as ONNX: the graph of tests/onnx_write.py up to the last Swish, then
Unsqueeze -> LSTM -> Squeeze, then the two heads on the LSTM's output.  The LSTM node follows the ONNX operator's definition: inputs
X, W [1][4m][H], R [1][4m][m], B [1][8m] = [Wb | Rb], sequence_lens, initial_h, initial_c, P; gate order i o f c; attributes hidden_size and
direction.  No mlagents-learn LSTM export has been seen, so this is the operator's definition and not a copy of a real file.
The protobuf classes are those of tests/onnx_write.py.  `variant` writes one of the graphs Policy.from_onnx must refuse."""
import numpy as np
from onnx_write import _classes, _tensor

VARIANTS = ("bidirectional", "reverse", "peepholes", "sequence_lens", "activations", "hidden_size", "two_cells", "not_after_swish")


def _to_onnx_gates(a, m):
    """torch's i f g o blocks -> ONNX's i o f c"""
    return np.concatenate([a[g * m:(g + 1) * m] for g in (0, 3, 1, 2)])


def write_lstm_actor(path, pol, variant=None):
    assert variant is None or variant in VARIANTS
    C = _classes()
    model = C["ModelProto"](ir_version=6, producer_name="pytorch", producer_version="1.7")
    model.opset_import.add(version=9)
    g = model.graph
    g.name = "torch-jit-export"
    count = [0]

    def tmp():
        count[0] += 1
        return str(count[0])

    def init(name, a):
        _tensor(g.initializer.add(), name, a)
        return name

    def node(op, ins, out=None, **attrs):
        out = out or tmp()
        n = g.node.add(op_type=op, name="%s_%d" % (op, len(g.node)))
        n.input.extend(ins)
        n.output.append(out)
        for k, v in attrs.items():
            a = n.attribute.add(name=k)
            if isinstance(v, float):
                a.f, a.type = v, 1
            elif isinstance(v, int):
                a.i, a.type = v, 2
            elif isinstance(v, bytes):
                a.s, a.type = v, 3                            # STRING
            elif v and isinstance(v[0], bytes):
                # STRINGS (field 9) is not among the fields of onnx_write's AttributeProto: its wire bytes are merged in as they are
                a.MergeFromString(b"".join(b"\x4a" + bytes([len(s)]) + s for s in v))
                a.type = 8
            else:
                a.ints.extend(v)
                a.type = 7
        return out

    m = pol.memory_size // 2
    init("version_number", np.array([3.0], np.float32))
    init("memory_size", np.array([float(pol.memory_size)], np.float32))
    x = "obs_0"
    if pol.norm_mean is not None:
        x = node("Sub", [x, init("network_body.observation_encoder.processors.0.normalizer.running_mean", pol.norm_mean)])
        x = node("Div", [x, init(tmp(), pol.norm_std)])
        x = node("Clip", [x], max=5.0, min=-5.0)
    x = node("Concat", [x], axis=1)
    pre = x
    for l, (W, b) in enumerate(zip(pol.W, pol.b)):
        k = "network_body._body_endoder.seq_layers.%d." % (2 * l)
        h = node("Gemm", [x, init(k + "weight", W), init(k + "bias", b)], alpha=1.0, beta=1.0, transB=1)
        x = node("Mul", [h, node("Sigmoid", [h])])
    L = pol.lstm
    W = _to_onnx_gates(L["W_ih"], m)[None]
    R = _to_onnx_gates(L["W_hh"], m)[None]
    B = np.concatenate([_to_onnx_gates(L["b_ih"], m), _to_onnx_gates(L["b_hh"], m)])[None]
    if variant == "bidirectional":
        W, R, B = np.concatenate([W, W]), np.concatenate([R, R]), np.concatenate([B, B])
    k = "network_body.lstm.lstm."
    seq = node("Unsqueeze", [pre if variant == "not_after_swish" else x], axes=[0])
    ins = [seq, init(k + "W", W), init(k + "R", R), init(k + "B", B),
           init(k + "seq_lens", np.ones(1, np.float32)) if variant == "sequence_lens" else "", "recurrent_in_h", "recurrent_in_c"]
    if variant == "peepholes":
        ins.append(init(k + "P", np.zeros((1, 3 * m), np.float32)))
    attrs = {"hidden_size": m + 1 if variant == "hidden_size" else m}
    if variant == "bidirectional":
        attrs["direction"] = b"bidirectional"
    elif variant == "reverse":
        attrs["direction"] = b"reverse"
    elif variant is None:
        attrs["direction"] = b"forward"
    if variant == "activations":
        attrs["activations"] = [b"HardSigmoid", b"Tanh", b"Tanh"]
    y = node("LSTM", ins, **attrs)
    if variant == "two_cells":
        y = node("LSTM", [y] + ins[1:], **attrs)
    x = node("Squeeze", [y], axes=[0, 1])
    c = "action_model._continuous_distribution."
    node("Gemm", [x, init(c + "mu.weight", pol.W_mu.reshape(1, -1)), init(c + "mu.bias", pol.b_mu)], "mu", alpha=1.0, beta=1.0, transB=1)
    init(c + "log_sigma", pol.log_sigma.reshape(1, 1))
    d = "action_model._discrete_distribution.branches.0."
    node("Gemm", [x, init(d + "weight", pol.W_branch), init(d + "bias", pol.b_branch)], "logits", alpha=1.0, beta=1.0, transB=1)
    with open(path, "wb") as f:
        f.write(model.SerializeToString())
    return path
