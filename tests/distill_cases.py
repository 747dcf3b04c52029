"""The seeded scenarios of the distillation tests that run models: the same numbers build them for the float64 CPU checks
of test_distill_host.py (where the seeds were picked, with the oracle's forward) and for the GPU tests."""
import numpy as np

from img2latex_amd import synth

PAD = 0
TINY = dict(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16))


def config(shape):
    V, E, H, L, attn = shape
    return synth.model_config(vocab_size=V, embedding_dim=E, hidden_dim=H, lstm_layers=L, attention=attn, **TINY)


# "It learns": the student, the one teacher and the batch.  alpha = 0: only the teacher's distribution is trained on; the
# hard targets are random tokens (none of them PAD, so all B x T positions are kept).
LEARN = dict(student=(16, 64, 64, 1, False), teacher=(16, 64, 64, 1, False), student_seed=31, teacher_seed=47,
             out_scale=4.0, B=4, T=8, steps=40, lr=3e-3, tau=2.0, alpha=0.0, eps=0.1)


def learn_case():
    """-> (student cfg, student sd, teacher cfg, teacher sd, images (B, 1, 16, 32) fp32, formulas (B, T + 1) int64)."""
    c = LEARN
    scfg, tcfg = config(c["student"]), config(c["teacher"])
    ssd = synth.make_state_dict(scfg, seed=c["student_seed"], out_scale=c["out_scale"], enc_scale=16.0)
    tsd = synth.make_state_dict(tcfg, seed=c["teacher_seed"], out_scale=c["out_scale"], enc_scale=16.0)
    images = synth.make_images(c["B"], scfg, seed=311)
    formulas = synth.randint(312, "distill.learn.formulas", (c["B"], c["T"] + 1), 1, c["student"][0]).astype(np.int64)
    return scfg, ssd, tcfg, tsd, images, formulas


# Wiring: per vocabulary a student and two teachers of other E / H / layers, one of the three with attention; B = 3, T = 9.
WIRING = {
    513: dict(student=(513, 256, 256, 1, False), teachers=((513, 64, 128, 2, True), (513, 36, 192, 1, False)), seed=61),
    3: dict(student=(3, 4, 64, 1, False), teachers=((3, 8, 128, 2, True), (3, 4, 64, 1, False)), seed=67),
}
WIRING_B, WIRING_T = 3, 9
# Self-distillation: the wiring students with an output layer scaled so that their distributions differ from one position
# to the next -- then a teacher read one position off shows (soft > 0.1 hard in float64, test_distill_host.py), and the
# seeds were picked for that: at the wiring case's own out_scale = 12 the rows are too alike (0.08 and 0.001 of hard).
SELF = {513: dict(seed=61, out_scale=40.0), 3: dict(seed=84, out_scale=100.0)}
SELF_TAU = 2.0


def self_case(V):
    """-> (cfg, sd, images, formulas) of the self-distillation student; batch and formulas are the wiring case's."""
    scfg = config(WIRING[V]["student"])
    _, _, images, formulas = wiring_case(V)
    return scfg, synth.make_state_dict(scfg, seed=SELF[V]["seed"], out_scale=SELF[V]["out_scale"], enc_scale=16.0), images, formulas


def wiring_case(V):
    """-> (student (cfg, sd), [teacher (cfg, sd)] x 2, images, formulas (B, T + 1) int64 with PAD positions)."""
    c = WIRING[V]
    scfg = config(c["student"])
    student = (scfg, synth.make_state_dict(scfg, seed=c["seed"], out_scale=12.0, enc_scale=16.0))
    teachers = []
    for i, shape in enumerate(c["teachers"]):
        tcfg = config(shape)
        teachers.append((tcfg, synth.make_state_dict(tcfg, seed=c["seed"] + 1 + i, out_scale=12.0, enc_scale=16.0)))
    images = synth.make_images(WIRING_B, scfg, seed=c["seed"] + 10)
    if V > 8:
        formulas = synth.make_formulas(WIRING_B, WIRING_T + 1, V, seed=c["seed"] + 11, min_len=4)
    else:       # make_formulas draws its body from [4, V): here any token of [0, V), 0 being PAD
        formulas = synth.randint(c["seed"] + 11, "distill.wiring.formulas", (WIRING_B, WIRING_T + 1), 0, V).astype(np.int64)
        formulas[:, 1] = 1                                   # every row keeps at least its first target
    return student, teachers, images, np.asarray(formulas, dtype=np.int64)
