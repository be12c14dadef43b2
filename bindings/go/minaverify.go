// Package minaverify: cgo binding of libminaverify.so for the Go operator (INTEGRATION.md section 2).
// Written next to the header it binds; not built in this repository (no Go toolchain there).
package minaverify

/*
#cgo LDFLAGS: -lminaverify
#include <stdlib.h>
#include "mina_verify.h"
*/
import "C"

import (
	"errors"
	"unsafe"
)

type Ctx struct{ p *C.mina_ctx }

func lastError() error { return errors.New(C.GoString(C.mina_last_error())) }

func New(device int) (*Ctx, error) {
	var p *C.mina_ctx
	if rc := C.mina_ctx_create(C.int(device), &p); rc != 0 {
		return nil, lastError()
	}
	return &Ctx{p}, nil
}

func (c *Ctx) Close() { C.mina_ctx_destroy(c.p) }

func (c *Ctx) SrsCreate(curve int, depth uint32) error {
	if rc := C.mina_srs_create(c.p, C.int(curve), C.uint32_t(depth)); rc != 0 {
		return lastError()
	}
	return nil
}

// SetStateDedup: the protocol-state leg of the context's Proof-of-State jobs hashes each distinct state of a job once (off by default; no result changes).
func (c *Ctx) SetStateDedup(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.mina_ctx_set_state_dedup(c.p, v); rc != 0 {
		return lastError()
	}
	return nil
}

// StateDedupStats: states that went through a deduplicated leg, the distinct ones among them, fingerprint collisions (since the mode was last switched on).
func (c *Ctx) StateDedupStats() (states, distinct, collisions uint64, err error) {
	var a, b, d C.uint64_t
	if rc := C.mina_ctx_state_dedup_stats(c.p, &a, &b, &d); rc != 0 {
		return 0, 0, 0, lastError()
	}
	return uint64(a), uint64(b), uint64(d), nil
}

// ConfigureDedupStates: the process-wide boundary (VerifyMinaState and its batch form) deduplicates the protocol states of each chunk; other flags are kept by the caller.
func ConfigureDedupStates(otherFlags uint32) { C.mina_verify_configure(C.uint32_t(otherFlags) | C.MINA_VERIFY_DEDUP_STATES) }

// ConfigurePackOnDevice: the process-wide boundary uploads each chunk's protocol-state bytes as they are and packs / pre-checks them on the GPU
// (mina_state_frontend_dev; bincode only); off by default, verdicts unchanged; other flags are kept by the caller.
func ConfigurePackOnDevice(otherFlags uint32) { C.mina_verify_configure(C.uint32_t(otherFlags) | C.MINA_VERIFY_PACK_ON_DEVICE) }

// ConfigureAccountOnDevice: VerifyAccountInclusion and its batch form upload a call's bytes as they are and run the whole Proof-of-Account job on the GPU
// (mina_account_job_dev; bincode only); off by default, verdicts unchanged; other flags are kept by the caller.
func ConfigureAccountOnDevice(otherFlags uint32) { C.mina_verify_configure(C.uint32_t(otherFlags) | C.MINA_VERIFY_ACCOUNT_ON_DEVICE) }

// ConfigureGroupedSearch: a chunk of the process-wide boundary whose folded check failed is searched for its culprits in groups of 64, from its staging in HBM
// (mina_ctx_set_search_groups, mina_state_job_each_dev); off by default, verdicts unchanged; other flags are kept by the caller.
func ConfigureGroupedSearch(otherFlags uint32) { C.mina_verify_configure(C.uint32_t(otherFlags) | C.MINA_VERIFY_GROUPED_SEARCH) }

// SetSearchGroups: the culprit search of the context's failed Proof-of-State jobs cuts a failing range into `groups` parts (2 .. 128) and checks all parts of a
// round in one pass on the job's lane; 0 (the default) keeps the fan search.
func (c *Ctx) SetSearchGroups(groups uint32) error {
	if rc := C.mina_ctx_set_search_groups(c.p, C.uint32_t(groups)); rc != 0 {
		return lastError()
	}
	return nil
}

// SetStreamBudget: the streams the context's pipelined device-resident jobs may keep busy (1 .. 31; <= 0: GPU_MAX_HW_QUEUES less the null stream's).  Decides
// between a fork per lane and the shared role streams; verdicts are the same either way.  Waits for what the context has queued.
func (c *Ctx) SetStreamBudget(n int) error {
	if rc := C.mina_ctx_set_stream_budget(c.p, C.int(n)); rc != 0 {
		return lastError()
	}
	return nil
}

// StreamPlanStats: the plan the context's last pipelined device-resident job was queued under: shared role streams or not, its state-hash streams (1 or 2),
// its chain pairs and the streams it keeps busy; all zero for a fork per lane and before the first such job.
func (c *Ctx) StreamPlanStats() (roles bool, carriers, sets, streams uint32, err error) {
	var r, a, b, d C.uint32_t
	if rc := C.mina_ctx_stream_plan_stats(c.p, &r, &a, &b, &d); rc != 0 {
		return false, 0, 0, 0, lastError()
	}
	return r != 0, uint32(a), uint32(b), uint32(d), nil
}

// SearchStats: legs searched in groups, their rounds and the parts checked, since the context was created.
func (c *Ctx) SearchStats() (searches, rounds, parts uint64, err error) {
	var a, b, d C.uint64_t
	if rc := C.mina_ctx_search_stats(c.p, &a, &b, &d); rc != 0 {
		return 0, 0, 0, lastError()
	}
	return uint64(a), uint64(b), uint64(d), nil
}

// SetSegFoldMfmaMin: segments of minLen proofs or more (and fewer than 2^17) of a segmented b_poly fold run on the matrix cores; 0 = never, 256 = the default.
func (c *Ctx) SetSegFoldMfmaMin(minLen uint32) error {
	if rc := C.mina_ctx_set_seg_fold_mfma_min(c.p, C.uint32_t(minLen)); rc != 0 {
		return lastError()
	}
	return nil
}

// SegFoldStats: segments the context folded on the matrix cores and with the VALU kernels (empty ones in neither), and its matrix-core passes.
func (c *Ctx) SegFoldStats() (mfmaSegments, valuSegments, mfmaPasses uint64, err error) {
	var a, b, d C.uint64_t
	if rc := C.mina_ctx_seg_fold_stats(c.p, &a, &b, &d); rc != 0 {
		return 0, 0, 0, lastError()
	}
	return uint64(a), uint64(b), uint64(d), nil
}

// SetMsmFusedTail: task-form MSMs queued after the call run bucket sums, reduction and finish as one launch (on) or as the staged kernels (off, the default).
func (c *Ctx) SetMsmFusedTail(on bool) error {
	v := 0
	if on {
		v = 1
	}
	if rc := C.mina_ctx_set_msm_fused_tail(c.p, C.int(v)); rc != 0 {
		return lastError()
	}
	return nil
}

// MsmTailStats: MSMs the context has queued with the fused tail and with the staged one.
func (c *Ctx) MsmTailStats() (fusedRuns, stagedRuns uint64, err error) {
	var a, b C.uint64_t
	if rc := C.mina_ctx_msm_tail_stats(c.p, &a, &b); rc != 0 {
		return 0, 0, lastError()
	}
	return uint64(a), uint64(b), nil
}

// SetFastInverse: MSMs queued after the call invert by batched divsteps at their finish (on) or by the power p - 2 (off, the default); the same bytes.
func (c *Ctx) SetFastInverse(on bool) error {
	v := 0
	if on {
		v = 1
	}
	if rc := C.mina_ctx_set_fast_inverse(c.p, C.int(v)); rc != 0 {
		return lastError()
	}
	return nil
}

// InverseStats: MSM finishes the context has queued with the divstep inversion and with the power.
func (c *Ctx) InverseStats() (gcdFinishes, fermatFinishes uint64, err error) {
	var a, b C.uint64_t
	if rc := C.mina_ctx_inverse_stats(c.p, &a, &b); rc != 0 {
		return 0, 0, lastError()
	}
	return uint64(a), uint64(b), nil
}

// SetChainInverse: the scalar stages of the wrap-proof chain and the Lagrange set-up queued after the call invert by batched divsteps (on) or by the power p - 2 (off, the default); the same bytes.
func (c *Ctx) SetChainInverse(on bool) error {
	v := 0
	if on {
		v = 1
	}
	if rc := C.mina_ctx_set_chain_inverse(c.p, C.int(v)); rc != 0 {
		return lastError()
	}
	return nil
}

// ChainInverseStats: launches of the kernels SetChainInverse covers that the context has queued in the divstep form and in the power form.
func (c *Ctx) ChainInverseStats() (gcdLaunches, fermatLaunches uint64, err error) {
	var a, b C.uint64_t
	if rc := C.mina_ctx_chain_inverse_stats(c.p, &a, &b); rc != 0 {
		return 0, 0, lastError()
	}
	return uint64(a), uint64(b), nil
}

// FieldInvGcd: n field inverses (32-byte little-endian elements, 0 -> 0) by the divstep iteration; the bytes of mina_field_inv.
func (c *Ctx) FieldInvGcd(field int, a []byte) ([]byte, error) {
	n := len(a) / 32
	out := make([]byte, n*32)
	if n == 0 {
		return out, nil
	}
	if rc := C.mina_field_inv_gcd(c.p, C.int(field), C.size_t(n), (*C.uint8_t)(unsafe.Pointer(&a[0])), (*C.uint8_t)(unsafe.Pointer(&out[0]))); rc != 0 {
		return nil, lastError()
	}
	return out, nil
}

// StateJobEachDev: per-proof verdicts (one uint32 each in dVerdicts) of a Proof-of-State job whose inputs are in HBM; waits for its lane.
func (c *Ctx) StateJobEachDev(jobs *C.mina_state_jobs, dVerdicts, dFlags unsafe.Pointer) error {
	if rc := C.mina_state_job_each_dev(c.p, jobs, dVerdicts, dFlags); rc != 0 {
		return lastError()
	}
	return nil
}

// MsmSegmentsDev: nseg variable-base MSMs over ranges [begin[s], end[s]) of one point / scalar array in HBM, one 68-byte record each (device pointers).
func (c *Ctx) MsmSegmentsDev(curve int, nTotal, nseg int, dBegin, dEnd, dBases, dScalars, dOut unsafe.Pointer) error {
	if rc := C.mina_msm_segments_dev(c.p, C.int(curve), C.size_t(nTotal), C.size_t(nseg), dBegin, dEnd, dBases, dScalars, dOut); rc != 0 {
		return lastError()
	}
	return nil
}

// BPolyFoldSegmentsDev: nseg weighted folds of challenge polynomials over ranges of one batch in HBM, 2^k scalars each (device pointers).
func (c *Ctx) BPolyFoldSegmentsDev(field int, k uint32, batch, nseg int, dBegin, dEnd, dChals, dWeights, dOut unsafe.Pointer) error {
	if rc := C.mina_b_poly_fold_segments_dev(c.p, C.int(field), C.uint32_t(k), C.size_t(batch), C.size_t(nseg), dBegin, dEnd, dChals, dWeights, dOut); rc != 0 {
		return lastError()
	}
	return nil
}

// SelftestFe29: one routine of the 9 x 29-bit layer (op = C.MINA_FE29_*) on rows of 73 uint32 words, 37 words out per row.  Test-facing: the caller owns the
// operand bounds, nothing is range-checked on the device.
func (c *Ctx) SelftestFe29(field, op int, rows []uint32) ([]uint32, error) {
	n := len(rows) / (C.MINA_FE29_IN_OPERANDS*9 + 1)
	out := make([]uint32, n*(C.MINA_FE29_OUT_RESULTS*9+1)+1)
	if n == 0 {
		return out[:0], nil
	}
	if rc := C.mina_selftest_fe29(c.p, C.int(field), C.int(op), C.size_t(n), (*C.uint32_t)(unsafe.Pointer(&rows[0])), (*C.uint32_t)(unsafe.Pointer(&out[0]))); rc != 0 {
		return nil, lastError()
	}
	return out[:len(out)-1], nil
}

// SelftestFe32: one routine of the 8 x 32 layer (op = C.MINA_FE32_*) on rows of 65 uint32 words, 33 words out per row.  Test-facing: raw words, the caller owns
// each routine's contract, nothing is range-checked on the device.
func (c *Ctx) SelftestFe32(field, op int, rows []uint32) ([]uint32, error) {
	n := len(rows) / (C.MINA_FE32_IN_OPERANDS*8 + 1)
	out := make([]uint32, n*(C.MINA_FE32_OUT_RESULTS*8+1)+1)
	if n == 0 {
		return out[:0], nil
	}
	if rc := C.mina_selftest_fe32(c.p, C.int(field), C.int(op), C.size_t(n), (*C.uint32_t)(unsafe.Pointer(&rows[0])), (*C.uint32_t)(unsafe.Pointer(&out[0]))); rc != 0 {
		return nil, lastError()
	}
	return out[:len(out)-1], nil
}

// SelftestIpaRows: the transcript stage of the opening check alone; the rows it leaves come back as canonical bytes in the caller's buffers (sizes: mina_verify.h).
// Test-facing: opt may be nil; side and offsets may be nil when no entry is shared.  flags = malformed word, lane form (16 / 8 / 3), side-stream word.
func (c *Ctx) SelftestIpaRows(curve int, openings []C.mina_ipa_opening, randBase, sgRandBase []byte, opt *C.mina_ipa_rows_options,
	points, scalars, chals, sigma, side []byte, offsets []uint32) (flags [3]uint32, err error) {
	var pSide *C.uint8_t
	var pOff *C.uint32_t
	if len(side) > 0 && len(offsets) > 0 {
		pSide, pOff = (*C.uint8_t)(unsafe.Pointer(&side[0])), (*C.uint32_t)(unsafe.Pointer(&offsets[0]))
	}
	rc := C.mina_selftest_ipa_rows(c.p, C.int(curve), C.size_t(len(openings)), &openings[0], (*C.uint8_t)(unsafe.Pointer(&randBase[0])), (*C.uint8_t)(unsafe.Pointer(&sgRandBase[0])), opt,
		(*C.uint8_t)(unsafe.Pointer(&points[0])), (*C.uint8_t)(unsafe.Pointer(&scalars[0])), (*C.uint8_t)(unsafe.Pointer(&chals[0])), (*C.uint8_t)(unsafe.Pointer(&sigma[0])),
		pSide, pOff, (*C.uint32_t)(unsafe.Pointer(&flags[0])))
	if rc != 0 {
		return flags, lastError()
	}
	return flags, nil
}

// AccumulatorCheckMulti: one deterministic verdict per proof (len(sg)/64 proofs).
func (c *Ctx) AccumulatorCheckMulti(curve int, k uint32, pre, sg []byte) ([]bool, error) {
	n := len(sg) / 64
	out := make([]byte, n)
	rc := C.mina_accumulator_check_multi(c.p, C.int(curve), C.uint32_t(k), C.size_t(n),
		(*C.uint8_t)(unsafe.Pointer(&pre[0])), (*C.uint8_t)(unsafe.Pointer(&sg[0])), (*C.uint8_t)(unsafe.Pointer(&out[0])))
	if rc != 0 {
		return nil, lastError()
	}
	v := make([]bool, n)
	for i := range out {
		v[i] = out[i] != 0
	}
	return v, nil
}

// VerifyMinaState: drop-in for the operator's cgo call of verify_mina_state_ffi (bincode MinaStateProof + MinaStatePubInputs).
func VerifyMinaState(proof, pub []byte) bool {
	if len(proof) == 0 || len(pub) == 0 {
		return false
	}
	return bool(C.mina_verify_state((*C.uint8_t)(unsafe.Pointer(&proof[0])), C.size_t(len(proof)), (*C.uint8_t)(unsafe.Pointer(&pub[0])), C.size_t(len(pub))))
}

// VerifyAccountInclusionFFI: drop-in for verify_account_inclusion_ffi (bincode MinaAccountProof + MinaAccountPubInputs).
func VerifyAccountInclusionFFI(proof, pub []byte) bool {
	if len(proof) == 0 || len(pub) == 0 {
		return false
	}
	return bool(C.mina_verify_account((*C.uint8_t)(unsafe.Pointer(&proof[0])), C.size_t(len(proof)), (*C.uint8_t)(unsafe.Pointer(&pub[0])), C.size_t(len(pub))))
}

// Queue: the completion queue (mina_verify_queue_*): Submit from any goroutine, one goroutine owns Wait and feeds a channel (INTEGRATION.md has the sketch).
type Queue struct{ p *C.mina_verify_queue }

// Completion: Tag is the submission's; Verdict is false whenever Rc != 0.
type Completion struct {
	Tag     uint64
	Verdict bool
	Rc      int
	Kind    uint8
}

func NewQueue(capacity, workers uint32) (*Queue, error) {
	var p *C.mina_verify_queue
	if rc := C.mina_verify_queue_create(C.uint32_t(capacity), C.uint32_t(workers), &p); rc != 0 {
		return nil, lastError()
	}
	return &Queue{p}, nil
}

// Close runs what is still pending, waits for it and frees the queue; no other call on the queue may be in flight.
func (q *Queue) Close() { C.mina_verify_queue_destroy(q.p) }

// Submit: the queue copies both slices before it returns.  accepted = false: every slot is held (MINA_ERR_FULL), take completions first.
func (q *Queue) Submit(kind uint32, proof, pub []byte, tag uint64, more bool) (accepted bool, err error) {
	var pp, qq *C.uint8_t
	if len(proof) > 0 {
		pp = (*C.uint8_t)(unsafe.Pointer(&proof[0]))
	}
	if len(pub) > 0 {
		qq = (*C.uint8_t)(unsafe.Pointer(&pub[0]))
	}
	flags := C.uint32_t(0)
	if more {
		flags = C.MINA_SUBMIT_MORE
	}
	rc := C.mina_verify_queue_submit(q.p, C.uint32_t(kind), pp, C.size_t(len(proof)), qq, C.size_t(len(pub)), C.uint64_t(tag), flags)
	if rc == C.MINA_ERR_FULL {
		return false, nil
	}
	if rc != 0 {
		return false, lastError()
	}
	return true, nil
}

func (q *Queue) Flush() { C.mina_verify_queue_flush(q.p) }

// Wait blocks until a completion is available or timeoutUs has passed (negative: for ever) and returns up to max of them.
func (q *Queue) Wait(max int, timeoutUs int64) []Completion {
	buf := make([]C.mina_verify_completion, max)
	var n C.size_t
	if max == 0 || C.mina_verify_queue_wait(q.p, &buf[0], C.size_t(max), &n, C.int64_t(timeoutUs)) != 0 {
		return nil
	}
	out := make([]Completion, int(n))
	for i := range out {
		out[i] = Completion{uint64(buf[i].tag), buf[i].verdict == 1, int(buf[i].rc), uint8(buf[i].kind)}
	}
	return out
}

// VerifyAccountInclusion: the Merkle part of verify_account_inclusion_ffi on the reference's byte contract.
func (c *Ctx) VerifyAccountInclusion(proof, pub, leafHash []byte) (bool, error) {
	var verdict C.uint8_t
	// the C side takes arrays of pointers: pin the two buffers in C memory for the call (cgo pointer rules)
	cp, cq := C.CBytes(proof), C.CBytes(pub)
	defer C.free(cp)
	defer C.free(cq)
	p, q := (*C.uint8_t)(cp), (*C.uint8_t)(cq)
	pl, ql := C.size_t(len(proof)), C.size_t(len(pub))
	rc := C.mina_verify_account_inclusion(c.p, 1, &p, &pl, &q, &ql, (*C.uint8_t)(unsafe.Pointer(&leafHash[0])), &verdict)
	if rc != 0 {
		return false, lastError()
	}
	return verdict == 1, nil
}
