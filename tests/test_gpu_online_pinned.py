"""Five online push entry points against the bytes of the build before their code was shared.

td_online_push, td_fc_online_push, td_cca_online_push and td_calib_online_push share their state layout, staging,
FIR prediction, per-frame score, window block and tail update through csrc/online_common.h; the fifth,
td_fccalib_online_push, takes its forward from the text td_fc_online_push includes (csrc/online_dnn_forward_body.h)
and its walk from the header td_calib_online_push includes (csrc/online_calib_common.h).  The other online
suites compare every cut of a recording with one push and with the batch kernels; this file pins the shared blocks
themselves: a fixed-seed recording (np.random.RandomState) goes through a sequence of pushes, and the SHA-256 of every
output -- per push the scores, the decisions, pred / proj and the per-frame scores, at the end the state bytes; for
the two calibrations the state bytes after every push -- is compared with PARENT_SHA256.

PARENT_SHA256 was produced once, by this file's own run_case, from the library of the parent commit 3f4d7ac ("Add an
online calibration: a decoder's statistics and LDA from pushes"), which holds the four kernels as four hand-kept
copies, selected through TD_HOTPATH_LIB on the MI355X; the digests of the DNNCALIB family the same way from the
library of 9a35557 ("Sweep the FIR and CCA projection kernels at their edges; fix NaN spread"), the last commit in
which dnn_calib_push_kernel holds its forward and its walk as hand-kept copies.  None is ever to be produced from the
code under test.

The cases are the smallest at which each shared block can go wrong, a few dozen combinations that between them touch:
channels 1, 3, 65, 128 (the 64-lane channel loop: one trip, one, two, the limit); context (0, 0), (2, 3), (0, 63) (no
tails, both, the lag limit); windows (1, 1), (5, 2) (the ring wraps inside a pass), (5, 9) (hop beyond width),
(100, 50) (a window longer than a pass: frames from the ring), (300, 7) (more than 256 frames: all four partial sums and
the stride loop); pushes of 1, pre + post - 1 (shorter than the tail: the shift through LDS), 64, 70 (two passes, the
second short), 0 rows with flush, and a flush that carries rows; decoders wta / stepped / none (the stepped state is in
the hashed state bytes and carries across pushes); reductions first / mean / mean-squared / lda (and the CCA's
second); 1 and 3 sessions with one shared model and with a model per session, the rows of a push a slice whose row
and session strides are larger than a row and a block; hidden layers [], [5], [64, 3]; c2 1 and 3, dims 1 and 5,
post1 != post2 both ways, pre2 != pre1; and the calibration at width 4 with pushes that end inside a window, exactly
on one and across two.  The DNN calibration's six: no hidden layer with those pushes; scalar chunk loads (w1 no
multiple of 4) and a model per session; the lag limit, the vector chunk path and a layer behind layer 1; a flush that
carries rows under one shared model; width 1 (every frame closes a window) at K = 8192; a window longer than a pass
over 70 + 1 + 300 rows."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# push lengths of a recording (T: pre + post - 1, dropped when it is not positive), then how it ends: None -- a flush
# without rows -- or the rows the flush carries
SEQS = {
    'A': (('1', 'T', '64', '70'), None),
    'B': (('70', '1'), 5),
    'L': (('1', 'T', '64', '70', '400'), None),          # long enough for windows of 100 and 300 frames
    'M': (('70', '1', '300'), 5),
    'W': (('2', '2', '7', '1'), None),                   # width 4, no delay: inside a window, on it, across two, on it
}

# (c, pre, post, width, hop, decoder, reduction, sessions, shared model, sequence)
LINEAR = [
    (1, 0, 0, 1, 1, 'wta', 'first', 1, True, 'A'),
    (3, 2, 3, 5, 2, 'stepped', 'mean', 3, False, 'A'),
    (65, 0, 63, 5, 9, 'none', 'mean-squared', 1, True, 'A'),
    (128, 2, 3, 100, 50, 'stepped', 'lda', 3, True, 'L'),
    (3, 0, 0, 300, 7, 'wta', 'lda', 1, True, 'L'),
    (65, 2, 3, 300, 7, 'stepped', 'first', 3, False, 'M'),
    (128, 0, 63, 5, 2, 'wta', 'mean', 1, True, 'B'),
    (1, 2, 3, 5, 9, 'stepped', 'mean-squared', 3, True, 'B'),
    (3, 0, 63, 1, 1, 'none', 'lda', 1, True, 'A'),
    (65, 0, 0, 100, 50, 'wta', 'first', 3, False, 'M'),
]
# (c, pre, post, hidden, width, hop, decoder, reduction, sessions, shared model, sequence)
DNN = [
    (1, 0, 0, (), 1, 1, 'wta', 'first', 1, True, 'A'),
    (3, 2, 3, (5,), 5, 2, 'stepped', 'mean', 3, False, 'A'),
    (65, 0, 63, (64, 3), 5, 9, 'none', 'mean-squared', 1, True, 'A'),
    (128, 2, 3, (5,), 100, 50, 'stepped', 'lda', 3, True, 'L'),
    (3, 0, 0, (64, 3), 300, 7, 'wta', 'lda', 1, True, 'L'),
    (128, 0, 63, (), 5, 2, 'wta', 'mean', 1, True, 'B'),
    (65, 2, 3, (), 300, 7, 'stepped', 'first', 3, False, 'M'),
    (1, 0, 63, (5,), 1, 1, 'stepped', 'mean-squared', 3, True, 'B'),
]
# (c1, pre1, post1, c2, pre2, post2, dims, width, hop, decoder, reduction, sessions, shared model, sequence)
CCA = [
    (1, 0, 0, 1, 0, 0, 1, 1, 1, 'wta', 'first', 1, True, 'A'),
    (3, 2, 3, 3, 1, 0, 5, 5, 2, 'stepped', 'mean', 3, False, 'A'),
    (65, 0, 63, 1, 0, 5, 5, 5, 9, 'none', 'mean-squared', 1, True, 'A'),
    (128, 2, 3, 3, 0, 7, 1, 100, 50, 'stepped', 'lda', 3, True, 'L'),
    (3, 0, 0, 3, 2, 3, 5, 300, 7, 'wta', 'lda', 1, True, 'L'),
    (65, 2, 3, 1, 2, 3, 5, 300, 7, 'stepped', 'second', 3, False, 'M'),
    (128, 0, 63, 3, 0, 0, 1, 5, 2, 'wta', 'mean', 1, True, 'B'),
    (1, 2, 3, 1, 0, 63, 1, 1, 1, 'stepped', 'first', 3, True, 'B'),
]
# (c, pre, post, width, sessions, shared model, sequence)
CALIB = [
    (3, 0, 0, 4, 1, True, 'W'),
    (1, 2, 3, 4, 3, False, 'A'),
    (65, 0, 63, 4, 1, True, 'A'),
    (128, 2, 3, 4, 3, True, 'B'),
    (128, 0, 63, 1, 1, True, 'B'),
    (3, 2, 3, 100, 3, False, 'M'),
]
# (c, pre, post, hidden, width, sessions, shared model, sequence)
DNNCALIB = [
    (3, 0, 0, (), 4, 1, True, 'W'),
    (1, 2, 3, (5,), 4, 3, False, 'A'),
    (65, 0, 63, (64, 3), 4, 1, True, 'A'),
    (128, 2, 3, (5,), 4, 3, True, 'B'),
    (128, 0, 63, (), 1, 1, True, 'B'),
    (3, 2, 3, (64, 3), 100, 3, False, 'M'),
]


def _name(case):
  return '-'.join('x'.join(str(u) for u in v) or 'none' if isinstance(v, tuple) else str(v) for v in case)


CASES = ([('linear-' + _name(c), 'linear', c) for c in LINEAR] + [('dnn-' + _name(c), 'dnn', c) for c in DNN] +
         [('cca-' + _name(c), 'cca', c) for c in CCA] + [('calib-' + _name(c), 'calib', c) for c in CALIB] +
         [('dnncalib-' + _name(c), 'dnncalib', c) for c in DNNCALIB])

# the parent commit's outputs: {case: {output: SHA-256}}
PARENT_SHA256 = {
    'linear-1-0-0-1-1-wta-first-1-True-A': {
        'scores': '316035388e88b21bea77bd911e853a650994de3a1cc70f99c4b3dfbf5d32e399',
        'decisions': 'f9db6d474ba2e951d49287ec3775b1094b7c5ef04224beab19e3756dcb41cc3a',
        'pred': 'e62d007305dfe69cb448486287fe63e7b69e8a0d040b2540184ae5c9077f1f42',
        'frame': '316035388e88b21bea77bd911e853a650994de3a1cc70f99c4b3dfbf5d32e399',
        'state': '0b024950e5c4cd6a5f7df45db392eae5588b5fb40afe5a062ae01962ed193c10',
    },
    'linear-3-2-3-5-2-stepped-mean-3-False-A': {
        'scores': 'b98ee40ef73b8cf1d5f548f6a23aa9062fdf763ef8dd7b1c43a6baa1bdd58356',
        'decisions': '08562fc69918bb1fa0dfe8c93468e40323999a14e870dcc7a89ddbfdec456459',
        'pred': 'bf88e74e41c34e170642128f831633305b403938b8376e6ed42b08e4577b22d5',
        'frame': 'a2fc550f5639564bf27d9deb2de82a33a821d5522749f105309d47f4c4229dfb',
        'state': '30d126444038bf4ed72e6f89f738cfbc06cce8034efca17ccf86f22855953173',
    },
    'linear-65-0-63-5-9-none-mean-squared-1-True-A': {
        'scores': '7295baff41a19ae45274588d25d64951f686abacb9fd0a262b64684908efc40e',
        'decisions': '6a4875ddaceaa91fb3369f0f6d962f77442daf1b1d97733457d12bcabdf79441',
        'pred': '98ae83f6ab09fe2dcde1b4b6dded0fe51da82c0fd1c766f2a00f8352cbbe10a6',
        'frame': 'c4e84286edae7b863792a35fae624167a343948d99d9334172afc61b6d4e6e96',
        'state': 'fe0d3907951c52f053ab668c3b4de40545d2bbc25abe8402505109f43b3c6b0e',
    },
    'linear-128-2-3-100-50-stepped-lda-3-True-L': {
        'scores': '08f7b967f6a3d83dbcd84d4dc96b22f7ca5c44726375ae603208fffebdd70006',
        'decisions': '6925bb588f5cbb7cd999525d1e7dc85227d77bfcb91373d07ecb0918afa1703f',
        'pred': '5a465b99adccdf5c9e14f5760c0ccde5f92fe80b357fd35c2c55a8e2e31961d8',
        'frame': '0efae9390f4df616a58eefd51fa8fee68375a7735bdda64cf0a91db9ef420a62',
        'state': 'cd470f1e34c2052791dd8c7d98f77a79f5697e89029ed4d43110f75275bee0c1',
    },
    'linear-3-0-0-300-7-wta-lda-1-True-L': {
        'scores': 'fa487730131172b518d7053e39026956189f61ee2c2f25e02cbd42547e42abcd',
        'decisions': '3564ee31af273c6d2d8f93bed6c21128bf257eb49ffd956ca08118410c44039e',
        'pred': '555dec9c83fc3b1b56012606f0817dff05c0d58d839a32d7c949bf7f9aecb263',
        'frame': '71bbc3ad23e580d3edcd3ca5307ecf7cde3f4f6655611186aa248a1f0b112186',
        'state': 'd375f015c68319bb0191b161af87d75a519c9a365b6627b6ba28c759d1a22274',
    },
    'linear-65-2-3-300-7-stepped-first-3-False-M': {
        'scores': 'a8251b4d2bf3277c3d15d02ab666de7af9d1f610789aa9ab1bc05ebfcc250d39',
        'decisions': '155d21fa832076e3deb612972d75b4d562fce232c75b07686fee85945453b577',
        'pred': '2398a40b86503ccb5cf78acd57aed3e29c068325495f84f5998fd25f8ef529f4',
        'frame': 'd760a23c4bd142b6017a5d35dc3070608af29fcdccbcce55d9f3180033c5e4a0',
        'state': 'e1ffad53c7baf907792617fd6d1cb62b50d7cc9c966a84258c6b2b43cc48177e',
    },
    'linear-128-0-63-5-2-wta-mean-1-True-B': {
        'scores': 'cf04bf5f6ec932ff2ff707b3da157f1d2cafd06c1ae797e1ddd6d2712ff8236a',
        'decisions': '8185dda597e8d742339528ea591437b9fbcfecf64ec34c6dc97c8148025303f5',
        'pred': '5b2a61a788ad4fcdacfe42b5c8d3b7b55506616ad90e3d82950c5c051ba1532d',
        'frame': '39fac646309530082e25208993315057d4d37bc48134c6320967c8b692755491',
        'state': 'fb02cd73b517807a4830d67f4ba860f6d5c1754b8be60d53748bad5ca822510a',
    },
    'linear-1-2-3-5-9-stepped-mean-squared-3-True-B': {
        'scores': '28ea6bda56ae94750a40800b9e06f7f888f741f63c6e466901a3ea7407e4eced',
        'decisions': '85526ba79728a470972be92942ef4de212630c9368703cb4ab3cb42dece95912',
        'pred': 'b75c8e0eaa987b68d45a385e6d8da03b016eca7db1f201b3f2323918b6a6529c',
        'frame': '29ffda4b1c1c025e182dd322e17a2776b16c68cf543a29d8d8841d7b51ff1942',
        'state': '8d419e27d8688299e596796681900c66033aac8fab92df16c1277198f36a8c6d',
    },
    'linear-3-0-63-1-1-none-lda-1-True-A': {
        'scores': '5f0759590cf293e8100828f622215d0884ad56432896031ffa82d91c183e7967',
        'decisions': '8ce53fa730feb908a84715dc714ab7b5db503ad7d093bddb3f8b7fcf3a84cd7b',
        'pred': 'c68e135774d7f3d12de07c1dde50052688a879091d96805538cc7371b8240b6f',
        'frame': '5f0759590cf293e8100828f622215d0884ad56432896031ffa82d91c183e7967',
        'state': '5df8be3c9146e99f6c0f91a1cc0caed72e72e20766b5cde893a19d8366085115',
    },
    'linear-65-0-0-100-50-wta-first-3-False-M': {
        'scores': 'b47ddb4a43fef5c8742db7f883a045bea7d077a69e6574cbd9e519c111bea277',
        'decisions': '4fdf549afcfd7ad176b62cf9b7f9b5f1afb73d6a41969af2f386b1db3c0b22d0',
        'pred': 'a4d7513b5086d3d44c5a02c5ec260473a381f16a6f9fe428b3003cbcd2943828',
        'frame': 'f299ba892bf091bb7fa4e828d3a45316dfbab6719b2d38d44a04ee2e4d50c888',
        'state': 'f6476fd740c98227d0c890808a2e9ffd969748978b7f1e68d8ddd27848a1ae2f',
    },
    'dnn-1-0-0-none-1-1-wta-first-1-True-A': {
        'scores': '01186f4d5c1b88e66d108c8d4b83c3a053bff5b0212d62afa1153c4f96dd5704',
        'decisions': '0f394ecca906ed781c5e35da0b9301986507ed64e75098b6adbce819eadb4ba2',
        'pred': 'fa6747484c6c76522918e79b5b8959222c14c3e5ced2e6bcbc1671f7f0399f27',
        'frame': '01186f4d5c1b88e66d108c8d4b83c3a053bff5b0212d62afa1153c4f96dd5704',
        'state': '936171a095563b0d088551538356bb6226e965806b7ffe888a3fe4ef058573c3',
    },
    'dnn-3-2-3-5-5-2-stepped-mean-3-False-A': {
        'scores': '896499f9c31def949fc5ab1cbb6b738ae428e04d529ffd3ea0ab041805eb7ca5',
        'decisions': 'cc859d4d468b457b39784e5d7956e974c8dcbf4b27d1d4d9eaa5934d5a9975e6',
        'pred': '98af57f071cc7d57fb33cd0482557960dcb1d8944b212a4e8f74075475c726c0',
        'frame': 'f7be8b6d19441882d8e524d2f14c7803dffd445f8ceec623c104a1ae1f4aa138',
        'state': 'a1085b4dc9ebc8c1823e7ee2fc9d4522afb8dcb58d93910ee2c3895f3cec90e7',
    },
    'dnn-65-0-63-64x3-5-9-none-mean-squared-1-True-A': {
        'scores': 'cdd17a2be04fe8c9aa8d8a159735b095e68c0bccf69f3590442d4491a5b9f1b5',
        'decisions': '6a4875ddaceaa91fb3369f0f6d962f77442daf1b1d97733457d12bcabdf79441',
        'pred': '01b07a70087546cd18cbacfa79e889d574b8ec2166a02a6fc79df88ca551cf1f',
        'frame': 'f12a9fc9551c621add93268e9738f4f5f0a25d226b0e8f907a9ca59aeef89d6d',
        'state': '01fdcd2b0da8b25f9fc970ca41f35804f5c1311f0e2ea0b12d3399ee52ae716c',
    },
    'dnn-128-2-3-5-100-50-stepped-lda-3-True-L': {
        'scores': '6ba00525a665c8a14a672dd8c063d85991e01243c4741a010c73528331b26b1d',
        'decisions': '077e3095f93bb57737007812a1eaa614523ce4e8286528b6d9846b931bc265fe',
        'pred': '0a59c9e47ca61285caa850f299b0b70d4da1d821f5fda166f464e93a52a331bf',
        'frame': '50f29b58236c80817482864adf1c18a86ed972be43a072f1418c0219f36c1f8f',
        'state': '735af5f5fc90528d481a54b95a795704868415b7f7d73296c9100265edd46dad',
    },
    'dnn-3-0-0-64x3-300-7-wta-lda-1-True-L': {
        'scores': 'bd780be5ffe324d04cfdc8ad1806492301892cf244ff0fa161aafa0793f5cfc6',
        'decisions': 'eb142b0cae0baa72a767ebc0823d1be94e14c5bfc52d8e417fc4302fceb6240c',
        'pred': '067df70962bb29ba23846f87f0f39b61d180fc2445c4d6320f04981f2569ddce',
        'frame': 'c63ec1db17428adaf2767aa4659c5c2af9768f8747fa22aaafb02d7a017aaf45',
        'state': 'f26d6efd0b9fece35ba03e7a8a47662440e6f597a6de6e700450b7024be1a541',
    },
    'dnn-128-0-63-none-5-2-wta-mean-1-True-B': {
        'scores': '266b641871303893cd99a78151036708a3eee1a9d316a2c0648d7dc0540126c8',
        'decisions': '5c3da89633ee3d240dec513af658500f69f701ef046d551db2807f0ec5dbd9d9',
        'pred': '284f200985600b21ff1fd0ea89fa503287c8b97cdd0eee9a8c445fb143b3494e',
        'frame': 'ef4a643cf4d937074c83723afa9e86990f7a88df412a0aa8b56afe3df1d7f8b2',
        'state': 'd8ce5047040175762a823490c3eddc50410790d82c6fb87a938d88cd41533fb4',
    },
    'dnn-65-2-3-none-300-7-stepped-first-3-False-M': {
        'scores': '4c341b2af2732d0ca5162cc9fb7e18ffb84c696506de8c3bcaed1818757edf16',
        'decisions': '7217321ff642d343416337be550b8be0f3cd0b2682117f7d5ab3feeb0225bb64',
        'pred': 'a86a84c610198a7110eba98522235ea2e224d53c48b5adcdd860e8474351ac74',
        'frame': '7d4b3d04c59607fa75333ff9e45b2538e86b2b69533480eea1dc26e88f5c6f47',
        'state': 'cb05de665886fbfe8456b8e6b643c31727bc0ed29abcc76c213d369a532d6083',
    },
    'dnn-1-0-63-5-1-1-stepped-mean-squared-3-True-B': {
        'scores': '71ef50d2dfbfecc69a1f23fed42eea2198a68036f5c7389b71a959fb54cc573d',
        'decisions': 'a5bb29b67f81eccd13fd3fff794871655543169df148a0b074592616fb25e895',
        'pred': '7decf02c4a4c0a505d002e9810ee7ae88500cc68bc4cea135f6636668f7d22dc',
        'frame': '71ef50d2dfbfecc69a1f23fed42eea2198a68036f5c7389b71a959fb54cc573d',
        'state': '74e10f052e154c6faf77e3dd61fdcd19fa312d5f32987c71ab50082db6c29ffb',
    },
    'cca-1-0-0-1-0-0-1-1-1-wta-first-1-True-A': {
        'scores': '61d453b832e41e4406ed9145aa14ea31efacef3bd98e8ab664fb714c1864ad51',
        'decisions': '52466ea730601f760caf327b851d8dfefc6de05d3e9655def8caca5b798e68aa',
        'pred': '1c40a7ceb7ee0bb32f88277459f53a5ac37cb924dadfbdea71ce1fdac69ce3fd',
        'frame': '61d453b832e41e4406ed9145aa14ea31efacef3bd98e8ab664fb714c1864ad51',
        'state': 'b3be71382f7191cd9d5c2b83cc4108e3f4ec1adc6fd7674ba57a0efcf1c2dcbc',
    },
    'cca-3-2-3-3-1-0-5-5-2-stepped-mean-3-False-A': {
        'scores': '9d9fc219d7ff6b8d90911cfc6dbdddbff2c2e230e0e3213110f7d8e00b822b45',
        'decisions': '312fbeb51cde1accdd60cf6168892ad3a37a5f361c7d2d2858e3d8f481a410c7',
        'pred': '5d843dedc25ec121a0a6ac2fed36868976cbf27d5c4f9b419e51914f9411809c',
        'frame': 'f5f08e20eb8869b4086778ca956ad66330c3ab8f78ecacdf8f49e26f3d30bf7b',
        'state': '907284a1ca41a81234a4a609b86fea4831efd8e63ccae8d138347b67e7807413',
    },
    'cca-65-0-63-1-0-5-5-5-9-none-mean-squared-1-True-A': {
        'scores': 'ec9d1275582769952dd6734fb8c7ff9a6a3ecaa7447710fabbb351d650a91a76',
        'decisions': '6a4875ddaceaa91fb3369f0f6d962f77442daf1b1d97733457d12bcabdf79441',
        'pred': 'bdb4017663f3290c25a9426358a13bf789bed380d70b7df00fe4982a7af30055',
        'frame': '7176506a90f02365240292688a36def76fa7817e74f2d3963f9d4d09e710e1b8',
        'state': '0fe8e88a52d51c232920bb08b5d2f097124a637ae3996725133bb2e6d2c5c7eb',
    },
    'cca-128-2-3-3-0-7-1-100-50-stepped-lda-3-True-L': {
        'scores': 'b9862413559d5ef64435dfe30ace311c42283fd8fcf9b05c4d43b03019a2feaa',
        'decisions': '68bbcca6ca9f14f705ce68489fb368681ddc5ca4d981d120bc42bfe9517632f3',
        'pred': '2bcdaf541aba16bf21fe4159d7ee8f5f9ec5bad64fbd34ccfa348a1d77c2eded',
        'frame': '584a82004722d8b5473e19396c0f0ce8a4a0a2702bb5bec0463361093de01439',
        'state': '3859554c0292f7c90df85d9fd86304b8febeed23697573ac96713c552baa355f',
    },
    'cca-3-0-0-3-2-3-5-300-7-wta-lda-1-True-L': {
        'scores': 'ad2eca94df76f45f2d743525abab0c7e221cebface0a9fef047e2da522673b9c',
        'decisions': 'eb142b0cae0baa72a767ebc0823d1be94e14c5bfc52d8e417fc4302fceb6240c',
        'pred': 'fd4b9548e8682e00a1920f7d9aa8254b65a950ece2c7ac659deb600faa885c8b',
        'frame': '2068a3c43a4a6d56983ff68be49792975bba2192bf47879612373ad5a3e69133',
        'state': '90599c27ee9d18c1d62ca2017b2e8404ed9011773c09c075591de589a1857623',
    },
    'cca-65-2-3-1-2-3-5-300-7-stepped-second-3-False-M': {
        'scores': '034c551395c47962c82351e8f7e41530f708c4a318dbad902b02fdb928a6e01f',
        'decisions': 'e696b175d3a1a9f5157e1959f8febfb424677b627d329d7ce6ec896837c77b98',
        'pred': '6f43ebf2cb7226130b657677c9a7ca432535464b87156b0f017d3763f11e6105',
        'frame': 'c2a85c3b7c26f6ca7fc1ac9c3a6c578e04b03a09d0110d77f165cf110acbbc14',
        'state': '21f67e7e2ae1c9baa1a2c7258766781bf493344e237198d40e9d702c4ae2e145',
    },
    'cca-128-0-63-3-0-0-1-5-2-wta-mean-1-True-B': {
        'scores': '98d72d4363cbca0ca1e92269f2e2c3e92b256c68592ef58375372d4f55a9ceac',
        'decisions': '5b658a181e49c5a718a6cf7fcda40bdebe380b66430d4ec2179df11c8e65f5fa',
        'pred': '5734a5fa5981bf983e038611873ca30f0fbba695f86ca096a4e3326bffd1e179',
        'frame': '51ea5e2fb1ea592e260e460c5d1801b525b3566fece88054c5d54de31bd8ec1c',
        'state': 'e4307d728b52d025f0698a3872897a27066707634a0418ef33b0ae53b11a1991',
    },
    'cca-1-2-3-1-0-63-1-1-1-stepped-first-3-True-B': {
        'scores': '184a450c41118462a143a4e36c9917c9b08f4bb1813eb70f96ec7dd448a3bdc0',
        'decisions': '60e2676d5916bc7cb6da85521c0050b71fd6dbc9c051ca02879f0b892d33c041',
        'pred': '736d7521e6addf3e608b33fbaa78f89e16f05a80a5849936ede1bd631fab3c5a',
        'frame': '184a450c41118462a143a4e36c9917c9b08f4bb1813eb70f96ec7dd448a3bdc0',
        'state': 'c75aa04a61f183b0b90d12382d8efaecce15429522a91fbad94c0e4f785538d1',
    },
    'calib-3-0-0-4-1-True-W': {
        'state': 'd89791a4fdbdf893a07875508f364e95bdd3a9c6ed4e52bccf89341e87af78b9',
    },
    'calib-1-2-3-4-3-False-A': {
        'state': 'af72601199a0ad79075d8234e14f5054990ed0546f42d65f5272fda43c23cd7d',
    },
    'calib-65-0-63-4-1-True-A': {
        'state': '49596273c96769c059e5b0a66e9e38395eafb8334e3643e3f257efa0cc5dbd01',
    },
    'calib-128-2-3-4-3-True-B': {
        'state': '5b4d0e66eaafd940214c5beb420d67f8742abc0c24772c532dac8a22ad7b20c2',
    },
    'calib-128-0-63-1-1-True-B': {
        'state': 'd7c1cf64e0b6f5db7a75710e87ee48b48ef029a877d71cecadc66aa4ff3a70c1',
    },
    'calib-3-2-3-100-3-False-M': {
        'state': 'a2c76e43b1b08747ba363a742443d2d8255fdaf40a91fe2ee1da3158d5d705f2',
    },
    'dnncalib-3-0-0-none-4-1-True-W': {
        'state': 'ff768dd2f74708c9736f2344fd57c85d22e1193c82083322d77bdf8206f29867',
    },
    'dnncalib-1-2-3-5-4-3-False-A': {
        'state': 'cd551f4df77dfa2b11dad3302d6cd78bfc22ec43526a8425ec9bbb9a0bedff64',
    },
    'dnncalib-65-0-63-64x3-4-1-True-A': {
        'state': 'e6c3a6006c0c5ea1d649149c1380a01b0e1453dcccd3a0f11c48f3238fd63176',
    },
    'dnncalib-128-2-3-5-4-3-True-B': {
        'state': '34c745f6c047f077b9b747bcbbd6c86dfdb77f1fb445148e76d1b5a7928e87b9',
    },
    'dnncalib-128-0-63-none-1-1-True-B': {
        'state': '8abef587d05a8b04955b880cf814d1e35bfae3e4eb26706164a6077d1a5ad648',
    },
    'dnncalib-3-2-3-64x3-100-3-False-M': {
        'state': '7030acd1f3c027de329ab6dafa98087784eb254e5b002fcbaf92e51564b08b48',
    },
}


def _lengths(seq, tail):
  lens, last = SEQS[seq]
  out = [tail - 1 if v == 'T' else int(v) for v in lens]
  return [n for n in out if n > 0], last


class _Recording(object):
  """Seeded rows on the device, handed out push by push as slices with a row stride of columns + 3 and a session
  stride of two rows more than the recording."""

  def __init__(self, rs, sessions, frames, columns):
    import torch
    self.at = 0
    self.full = [torch.from_numpy(rs.standard_normal((sessions, frames + 2, c + 3)).astype(np.float32)).to('cuda')
                 for c in columns]
    self.columns = columns

  def take(self, n):
    out = [t[:, self.at:self.at + n, :c] for t, c in zip(self.full, self.columns)]
    self.at += n
    return out


def _up(a):
  import torch
  return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _stats(rs, shape):
  """{mean_truth, mean_pred, power} along the axis of 3: small means, a power well away from zero."""
  s = 0.1 * rs.standard_normal(shape)
  s[..., 2, :] = 0.5 + np.abs(s[..., 2, :])
  return s


class _Hashes(object):
  def __init__(self, names):
    self.h = dict((n, hashlib.sha256()) for n in names)

  def add(self, name, tensor):
    self.h[name].update(tensor.cpu().numpy().tobytes())

  def digests(self):
    return dict((n, h.hexdigest()) for n, h in self.h.items())


def _run_decoder(dev, kind, case, rs):
  import torch
  if kind == 'cca':
    c1, pre1, post1, c2, pre2, post2, dims, width, hop, decoder, reduction, sessions, shared, seq = case
    post, tail = max(post1, post2), pre1 + max(post1, post2)
    k1, k2 = c1 * (pre1 + 1 + post1), c2 * (pre2 + 1 + post2)
    columns = (c1, c2, c2)
    sbytes = dev.cca_online_state_bytes(c1, pre1, post1, c2, pre2, post2, width)
  else:
    if kind == 'dnn':
      c, pre, post, hidden, width, hop, decoder, reduction, sessions, shared, seq = case
    else:
      c, pre, post, width, hop, decoder, reduction, sessions, shared, seq = case
    tail, k = pre + post, c * (pre + 1 + post)
    columns = (c, 2)
    sbytes = dev.online_state_bytes(c, pre, post, width)
  lens, last = _lengths(seq, tail)
  rec = _Recording(rs, sessions, sum(lens) + (last or 0), columns)
  models = 1 if shared else sessions
  if kind == 'cca':
    model = [_up((0.3 * rs.standard_normal(s)).astype(np.float32))
             for s in ((models, k1), (models, k1, dims), (models, k2), (models, k2, dims))]
    corr = _up(_stats(rs, (sessions, 2, 3, dims)))
    lda = _up(rs.standard_normal((sessions, dims + 2))) if reduction == 'lda' else None
  else:
    if kind == 'dnn':
      model = [_up((0.3 * rs.standard_normal((models, dev.dnn_param_count(k, hidden)))).astype(np.float32))]
    else:
      model = [_up((0.3 * rs.standard_normal((models, k))).astype(np.float32)),
               _up(rs.standard_normal(models).astype(np.float32))]
    corr = _up(_stats(rs, (sessions, 2, 3, 1))[..., 0])
    lda = _up(rs.standard_normal((sessions, 3))) if reduction == 'lda' else None
  state = torch.zeros((sessions, sbytes), dtype=torch.uint8, device='cuda')
  out = _Hashes(('scores', 'decisions', 'pred', 'frame', 'state'))
  pushed = 0
  for n, flush in [(n, False) for n in lens] + [(last or 0, True)]:
    rows = rec.take(n) if n else [None] * len(columns)
    common = dict(reduction=reduction, lda=lda, decoder=decoder, flush=flush, want_frames=True)
    if kind == 'cca':
      r = dev.cca_online_push(rows[0], rows[1], rows[2], model[0], model[1], model[2], model[3], corr, state, pushed,
                              pre1, post1, pre2, post2, width, hop, **common)
    elif kind == 'dnn':
      r = dev.dnn_online_push(rows[0], rows[1], model[0], list(hidden), corr, state, pushed, pre, post, width, hop,
                              **common)
    else:
      r = dev.online_push(rows[0], rows[1], model[0], model[1], corr, state, pushed, pre, post, width, hop, **common)
    pushed += n
    out.add('scores', r.scores)
    out.add('decisions', r.decisions)
    out.add('pred', r.proj if kind == 'cca' else r.pred)
    out.add('frame', r.frame)
  assert r.plan.emitted_after == pushed                    # (flushed: every frame is out)
  out.add('state', state)
  return out.digests()


def _run_calib(dev, kind, case, rs):
  import torch
  if kind == 'dnncalib':
    c, pre, post, hidden, width, sessions, shared, seq = case
  else:
    c, pre, post, width, sessions, shared, seq = case
  lens, last = _lengths(seq, pre + post)
  rec = _Recording(rs, sessions, sum(lens) + (last or 0), (c, 2))
  models, k = 1 if shared else sessions, c * (pre + 1 + post)
  if kind == 'dnncalib':
    params = _up((0.3 * rs.standard_normal((models, dev.dnn_param_count(k, hidden)))).astype(np.float32))
    sbytes = dev.online_dnn_calib_state_bytes(c, pre, post)
  else:
    w = _up((0.3 * rs.standard_normal((models, k))).astype(np.float32))
    b = _up(rs.standard_normal(models).astype(np.float32))
    sbytes = dev.online_calib_state_bytes(c, pre, post)
  state = torch.zeros((sessions, sbytes), dtype=torch.uint8, device='cuda')
  out = _Hashes(('state',))
  pushed = 0
  for n, flush in [(n, False) for n in lens] + [(last or 0, True)]:
    rows = rec.take(n) if n else [None, None]
    if kind == 'dnncalib':
      pushed = dev.online_dnn_calib_push(rows[0], rows[1], params, list(hidden), state, pushed, pre, post, width,
                                         flush=flush)
    else:
      pushed = dev.online_calib_push(rows[0], rows[1], w, b, state, pushed, pre, post, width, c=c, flush=flush)
    out.add('state', state)                                # (after every push: where a window ends matters)
  return out.digests()


def run_case(dev, name, kind, case):
  """{output: SHA-256} of one case; the seed is the case's place in CASES."""
  rs = np.random.RandomState(20261 + [c[0] for c in CASES].index(name))
  return _run_calib(dev, kind, case, rs) if kind in ('calib', 'dnncalib') else _run_decoder(dev, kind, case, rs)


@pytest.fixture(scope='module')
def dev():
  from telluride_decoding_amd import device
  return device


@pytest.mark.parametrize('name,kind,case', CASES, ids=[c[0] for c in CASES])
def test_every_output_has_the_parents_bytes(dev, name, kind, case):
  got = run_case(dev, name, kind, case)
  for output in sorted(got):
    print('%s %s %s' % (name, output, got[output]))
  assert got == PARENT_SHA256[name]
