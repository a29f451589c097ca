"""The surface of the sparse stack that a layout change must leave alone: the sparse names of the package namespace and
the ordered `state_dict` keys of the encoders — plain, after `convert_norm()`, after `.eval().fuse()` — against
tests/golden/sparse_surface.json, recorded before the Python side was split into layers; and the layering itself: nothing below
sparse_encoder.py imports it, and no module of the stack imports inside a function."""
import ast
import json
import os

import pytest

import mmdet3d_gaussian_amd as amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sparse_surface.json')
MODULES = ('sparse_tensor', 'sparse_conv', 'sparse_bn', 'sparse_pool', 'sparse_encoder')
ENCODER = dict(in_channels=4, sparse_shape=(9, 12, 10), base_channels=4, output_channels=8, encoder_channels=((4,), (8, 8), (8, 8)),
               encoder_paddings=((1,), (1, 1), (1, 1)))
UNET = dict(ENCODER, decoder_channels=((8, 8, 8), (8, 8, 4), (4, 4, 4)), decoder_paddings=((1, 0), (1, 0), (0, 1)))


def sparse_names():
    """the names of `amd.__all__` that one of MODULES defines, in `__all__`'s order"""
    return [n for n in amd.__all__ if getattr(getattr(amd, n), '__module__', '').rsplit('.', 1)[-1] in MODULES]


def state_dict_keys():
    keys = {}
    for block_type in ('conv_module', 'basicblock'):
        for form, step in (('plain', lambda m: m), ('convert_norm', lambda m: m.convert_norm()), ('eval_fuse', lambda m: m.eval().fuse())):
            keys[f'SparseEncoder/{block_type}/{form}'] = list(step(amd.SparseEncoder(block_type=block_type, **ENCODER)).state_dict())
    keys['MlvlSparseEncoder'] = list(amd.MlvlSparseEncoder(**ENCODER).state_dict())
    keys['SparseUNet'] = list(amd.SparseUNet(**UNET).state_dict())
    return keys


def surface():
    return dict(names=sparse_names(), state_dict=state_dict_keys())


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_sparse_names_of_the_package(golden):
    assert sparse_names() == golden['names']


def test_state_dict_keys_and_their_order(golden):
    got = state_dict_keys()
    assert sorted(got) == sorted(golden['state_dict'])
    for name, keys in got.items():
        assert keys == golden['state_dict'][name], name


def _tree(module):
    with open(os.path.join(os.path.dirname(amd.__file__), module + '.py')) as f:
        return ast.parse(f.read())


def _imported(node):
    """the module paths an Import / ImportFrom node names, dots of a relative import included"""
    if isinstance(node, ast.Import):
        return [a.name for a in node.names]
    base = '.' * node.level + (node.module or '')
    return [base] + [f'{base}.{a.name}' if node.module else base + a.name for a in node.names]


@pytest.mark.parametrize('module', ['sparse_tensor', 'sparse_conv', 'sparse_bn', 'sparse_pool'])
def test_nothing_below_the_encoder_imports_it(module):
    for node in ast.walk(_tree(module)):
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            assert not any('sparse_encoder' in path for path in _imported(node)), (module, node.lineno)


@pytest.mark.parametrize('module', MODULES)
def test_no_import_inside_a_function(module):
    for scope in ast.walk(_tree(module)):
        if isinstance(scope, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            for node in ast.walk(scope):
                assert not isinstance(node, (ast.Import, ast.ImportFrom)), (module, node.lineno)
