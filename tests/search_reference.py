"""The plainest restatement of the decoder's beam search (asr_hip/search.py:beam_search), the yardstick of tests/test_search_host.py:
one utterance at a time, one hypothesis at a time, no rows, no step object.  Python floats only; joint CTC scoring takes its prefix
scores from tests/ctc_prefix_reference.py, one (T,2) state carried by every hypothesis.

  logp(prefix) -> the V log-probabilities of the next label after `prefix` (a list of ids that starts with SOS)
"""
import math

import ctc_prefix_reference as R

PAD, SOS, EOS = 0, 1, 2
STEPS = 300


def best_first(values):
    """Indices of `values`, largest value first; equal values keep their index order."""
    return sorted(range(len(values)), key=lambda n: values[n], reverse=True)


def search_utterance(logp, W, frames, ctc=None):
    """-> the finished hypotheses of one utterance in the order they finished: dictionaries with 'score' and 'yseq' (and 'att', 'psi'
    under CTC).  frames: encoder frames of the (padded) batch; the step numbered frames - 1 ends every hypothesis it keeps with EOS.
    ctc = (mu, K, lp_u (T,V) float64 log-probabilities of the CTC head, T_u true frames of this utterance)."""
    first = {'score': 0.0, 'yseq': [SOS]}
    if ctc is not None:
        mu, K, lp_u, T_u = ctc
        first.update(att=0.0, psi=0.0, state=R.init_state(lp_u[None], [T_u], [0])[0])
    beam, finished = [first], []
    for n in range(STEPS):
        kept = []
        for hyp in beam:
            lp = logp(hyp['yseq'])
            order = best_first(lp)
            if ctc is None:
                for v in order[:W]:
                    kept.append({'score': hyp['score'] + lp[v], 'yseq': hyp['yseq'] + [v]})
            else:
                top = order[:K]
                last = hyp['yseq'][-1]
                psi, states = R.step(lp_u[None], [T_u], hyp['state'][None], [0], [last], [last == SOS], [top])
                psi = [float(x) for x in psi[0]]
                joint = []
                for k, v in enumerate(top):
                    if psi[k] == -math.inf:          # ruled out by CTC; no inf - inf
                        joint.append(-math.inf)
                    else:
                        joint.append((1.0 - mu) * lp[v] + mu * (psi[k] - hyp['psi']))
                for k in best_first(joint)[:W]:
                    kept.append({'score': hyp['score'] + joint[k], 'yseq': hyp['yseq'] + [top[k]], 'att': hyp['att'] + lp[top[k]],
                                 'psi': psi[k], 'state': states[0, k]})
            # the quirk: the list is cut back to W after EVERY hypothesis, not once after all of them
            kept = [kept[m] for m in best_first([h['score'] for h in kept])[:W]]
        if n == frames - 1:
            for hyp in kept:
                hyp['yseq'] = hyp['yseq'] + [EOS]
        beam = []
        for hyp in kept:
            (finished if hyp['yseq'][-1] == EOS else beam).append(hyp)
        if not beam:
            break
    return finished
