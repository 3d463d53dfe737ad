// Package gpbcbn254 mirrors the gnark-crypto bn254 calls used by mmsyan/GoPairingBasedCryptography and runs them on
// MI355X GPUs through the C ABI of libgpbc_bn254.so (include/gpbc_bn254.h).
//
// gnark's in-memory structs are the ABI buffers: fp.Element is [4]uint64 Montgomery little-endian, so a
// []bn254.G1Affine is already the 64-byte-stride array the library reads (unsafe.SliceData) and results land directly
// in bn254.GT / G1Affine / G2Affine values.  There is one code path: no call falls back to gnark's CPU arithmetic.
//
// NOT COMPILED in the build image of this repository (no Go toolchain there); the same surface is compiled and tested
// as C++ (include/gpbc_bn254.hpp, tests/cpp/*.cpp) and as Python ctypes (gopairingbasedcryptography_amd/bn254.py).
// INTEGRATION.md maps every function to the reference call sites it replaces.
package gpbcbn254

/*
#cgo CFLAGS: -I${SRCDIR}/../include
#cgo LDFLAGS: -L${SRCDIR}/../gopairingbasedcryptography_amd -lgpbc_bn254 -Wl,-rpath,${SRCDIR}/../gopairingbasedcryptography_amd
#include "gpbc_bn254.h"
#include "gpbc_bn254_hash.h"
#include "gpbc_bn254_share.h"
#include "gpbc_bn254_indexed.h"
#include "gpbc_bn254_select.h"
#include "gpbc_bn254_verify.h"
*/
import "C"

import (
	"errors"
	"math/big"
	"runtime"
	"sync"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254"
	"github.com/consensys/gnark-crypto/ecc/bn254/fp"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
)

var errSizes = errors.New("invalid inputs sizes") // gnark's own error text for Pair / PairingCheck

// gpbc_last_error() is thread-local on the C side and a goroutine may move to another OS thread between two cgo calls, so
// every exported function pins its goroutine for the length of the call (`defer pin()()` first thing): the status of a
// library call and the message that belongs to it are then read on the same thread.
func pin() func() {
	runtime.LockOSThread()
	return runtime.UnlockOSThread
}

func status(rc C.int) error {
	if rc == 0 {
		return nil
	}
	return errors.New(C.GoString(C.gpbc_last_error()))
}

func must(rc C.int) {
	if rc != 0 {
		panic("gpbcbn254: " + C.GoString(C.gpbc_last_error())) // gnark's methods cannot fail: surface engine errors loudly
	}
}

// Init binds the process to the given HIP devices (nil or empty: every visible device).  Host-slice batch calls then
// shard their index range over all of them inside the library; results do not depend on the number of devices.
func Init(devices []int) error {
	defer pin()()
	if len(devices) == 0 {
		n := int(C.gpbc_device_count())
		if n <= 0 {
			return errors.New(C.GoString(C.gpbc_last_error()))
		}
		for i := 0; i < n; i++ {
			devices = append(devices, i)
		}
	}
	d := make([]C.int, len(devices))
	for i, v := range devices {
		d[i] = C.int(v)
	}
	return status(C.gpbc_init_devices(&d[0], C.int(len(d))))
}

// NumDevices is the number of GPUs bound by Init.
func NumDevices() int { return int(C.gpbc_num_devices()) }

// InitCollectives opens one RCCL communicator over the bound devices: the partial sums of G1ScalarMulSum / G2ScalarMulSum
// are then exchanged by ncclAllGather over xGMI instead of through the host.
func InitCollectives() error {
	defer pin()()
	return status(C.gpbc_comm_init_all())
}

// Shutdown releases the library's device memory and communicators.
func Shutdown() error {
	defer pin()()
	destroyGeneratorTables() // before the devices go: the tables live in their HBM
	return status(C.gpbc_shutdown())
}

// Pair replaces bn254.Pair (cpabe/bsw07/bsw07_cpabe.go:75,184; access/tree/access_tree_node.go:106,110,119;
// bibe/afp25_bibe/afp25_bibe.go:227,395,399,403; ...): product of pairings, one final exponentiation.
func Pair(P []bn254.G1Affine, Q []bn254.G2Affine) (bn254.GT, error) {
	defer pin()()
	var gt bn254.GT
	if len(P) == 0 || len(P) != len(Q) {
		return gt, errSizes
	}
	seg := [2]C.uint64_t{0, C.uint64_t(len(P))}
	rc := C.gpbc_multi_pair(unsafe.Pointer(unsafe.SliceData(P)), unsafe.Pointer(unsafe.SliceData(Q)),
		&seg[0], 1, unsafe.Pointer(&gt))
	return gt, status(rc)
}

// PairingCheck replaces bn254.PairingCheck (signature/bls01_signature/bls_signature.go:81).
func PairingCheck(P []bn254.G1Affine, Q []bn254.G2Affine) (bool, error) {
	defer pin()()
	if len(P) == 0 || len(P) != len(Q) {
		return false, errSizes
	}
	seg := [2]C.uint64_t{0, C.uint64_t(len(P))}
	var ok C.uint8_t
	rc := C.gpbc_pairing_check(unsafe.Pointer(unsafe.SliceData(P)), unsafe.Pointer(unsafe.SliceData(Q)), &seg[0], 1, &ok)
	return ok == 1, status(rc)
}

// PairBatch is the batched form the engine adds: out[i] = Pair([P[i]], [Q[i]]).
func PairBatch(P []bn254.G1Affine, Q []bn254.G2Affine) ([]bn254.GT, error) {
	defer pin()()
	if len(P) == 0 || len(P) != len(Q) {
		return nil, errSizes
	}
	out := make([]bn254.GT, len(P))
	rc := C.gpbc_pair_batch(unsafe.Pointer(unsafe.SliceData(P)), unsafe.Pointer(unsafe.SliceData(Q)),
		C.size_t(len(P)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// MultiPair: out[j] = Pair(P[segOff[j]:segOff[j+1]], Q[segOff[j]:segOff[j+1]]) — the products the reference assembles
// from single pairings, GT.Mul / Div / Exp (ibe/bb04_ibe/bb04_ibe.go:213-225, access/tree/access_tree_node.go:106-157,
// bibe/afp25_bibe/afp25_bibe.go:395-413) with one final exponentiation per segment.
func MultiPair(P []bn254.G1Affine, Q []bn254.G2Affine, segOff []uint64) ([]bn254.GT, error) {
	defer pin()()
	if len(segOff) < 2 || len(P) != len(Q) || segOff[len(segOff)-1] != uint64(len(P)) {
		return nil, errSizes
	}
	out := make([]bn254.GT, len(segOff)-1)
	var p, q unsafe.Pointer
	if len(P) > 0 {
		p, q = unsafe.Pointer(unsafe.SliceData(P)), unsafe.Pointer(unsafe.SliceData(Q))
	}
	rc := C.gpbc_multi_pair(p, q, (*C.uint64_t)(unsafe.SliceData(segOff)), C.size_t(len(out)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// PairFixedQ: out[j] = Pair(P[j*m:(j+1)*m], Q) for one shared list Q of m points (a BSW07 key against many ciphertexts:
// access/tree/access_tree_node.go:106-119 under cpabe/bsw07/bsw07_cpabe.go:172-195; gnark: PrecomputeLines).
func PairFixedQ(P []bn254.G1Affine, Q []bn254.G2Affine) ([]bn254.GT, error) {
	defer pin()()
	if len(Q) == 0 || len(P) == 0 || len(P)%len(Q) != 0 {
		return nil, errSizes
	}
	out := make([]bn254.GT, len(P)/len(Q))
	rc := C.gpbc_multi_pair_fixed_q(unsafe.Pointer(unsafe.SliceData(P)), unsafe.Pointer(unsafe.SliceData(Q)),
		C.size_t(len(Q)), C.size_t(len(out)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// scalarBytes: big.Int -> 32-byte little-endian, reduced mod r (call sites pass fr.Element.BigInt values or rand.Int(r)).
func scalarBytes(s *big.Int, dst *[32]byte) {
	var t big.Int
	t.Mod(s, fr.Modulus())
	b := t.Bytes() // big-endian, at most 32 bytes after the reduction
	for i := range b {
		dst[len(b)-1-i] = b[i]
	}
}

// G1ScalarMultiplication replaces new(bn254.G1Affine).ScalarMultiplication(a, s)
// (signature/bls01_signature/bls_signature.go:45; cpabe/bsw07/bsw07_cpabe.go:69,149,157,160).
func G1ScalarMultiplication(p, a *bn254.G1Affine, s *big.Int) *bn254.G1Affine {
	defer pin()()
	var k [32]byte
	scalarBytes(s, &k)
	var out bn254.G1Affine // a and p may alias
	must(C.gpbc_g1_scalar_mul_batch(unsafe.Pointer(a), 1, unsafe.Pointer(&k[0]), 1, unsafe.Pointer(&out)))
	*p = out
	return p
}

// Fixed-base window tables of the two generators (1 MB / 2 MB of HBM), built on the first ScalarMultiplicationBase call:
// 32 mixed additions per multiplication instead of the variable-base kernel's doublings.
// A mutex, not a sync.Once: a Once whose function panics (a call before Init, a failed table build) is spent for good and would leave
// nil handles behind for every later call.  The handles are set only when both tables exist, a failed attempt is retried by the
// next call, and Shutdown destroys them so that Init after Shutdown builds fresh ones.
var (
	genMu            sync.Mutex
	g1Table, g2Table *C.gpbc_fixed_base
)

func generatorTables() (*C.gpbc_fixed_base, *C.gpbc_fixed_base) {
	genMu.Lock()
	defer genMu.Unlock()
	if g1Table == nil || g2Table == nil {
		_, _, g1, g2 := bn254.Generators()
		var t1, t2 *C.gpbc_fixed_base
		must(C.gpbc_g1_fixed_base_create(unsafe.Pointer(&g1), 1, &t1))
		if rc := C.gpbc_g2_fixed_base_create(unsafe.Pointer(&g2), 1, &t2); rc != 0 {
			msg := C.GoString(C.gpbc_last_error())
			C.gpbc_fixed_base_destroy(t1)
			panic("gpbcbn254: " + msg)
		}
		g1Table, g2Table = t1, t2
	}
	return g1Table, g2Table
}

func destroyGeneratorTables() {
	genMu.Lock()
	defer genMu.Unlock()
	if g1Table != nil {
		C.gpbc_fixed_base_destroy(g1Table)
	}
	if g2Table != nil {
		C.gpbc_fixed_base_destroy(g2Table)
	}
	g1Table, g2Table = nil, nil
}

// G1ScalarMultiplicationBase replaces new(bn254.G1Affine).ScalarMultiplicationBase(s)
// (cpabe/bsw07/bsw07_cpabe.go:69; bibe/afp25_bibe/afp25_bibe.go:160).
func G1ScalarMultiplicationBase(p *bn254.G1Affine, s *big.Int) *bn254.G1Affine {
	defer pin()()
	t1, _ := generatorTables()
	var k [32]byte
	scalarBytes(s, &k)
	must(C.gpbc_fixed_base_msm(t1, unsafe.Pointer(&k[0]), 1, unsafe.Pointer(p)))
	return p
}

// G2ScalarMultiplication replaces new(bn254.G2Affine).ScalarMultiplication(a, s)
// (signature/bls01_signature/bls_signature.go:63; cpabe/bsw07/bsw07_cpabe.go:73,83,103-121).
func G2ScalarMultiplication(p, a *bn254.G2Affine, s *big.Int) *bn254.G2Affine {
	defer pin()()
	var k [32]byte
	scalarBytes(s, &k)
	var out bn254.G2Affine
	must(C.gpbc_g2_scalar_mul_batch(unsafe.Pointer(a), 1, unsafe.Pointer(&k[0]), 1, unsafe.Pointer(&out)))
	*p = out
	return p
}

// G2ScalarMultiplicationBase replaces new(bn254.G2Affine).ScalarMultiplicationBase(s)
// (cpabe/bsw07/bsw07_cpabe.go:73; bibe/afp25_bibe/afp25_bibe.go:164-165).
func G2ScalarMultiplicationBase(p *bn254.G2Affine, s *big.Int) *bn254.G2Affine {
	defer pin()()
	_, t2 := generatorTables()
	var k [32]byte
	scalarBytes(s, &k)
	must(C.gpbc_fixed_base_msm(t2, unsafe.Pointer(&k[0]), 1, unsafe.Pointer(p)))
	return p
}

func frBytes(s []fr.Element) [][32]byte {
	k := make([][32]byte, len(s))
	for i := range s {
		var b big.Int
		scalarBytes(s[i].BigInt(&b), &k[i])
	}
	return k
}

// G1ScalarMultiplicationBatch: out[i] = [s[i]] bases[i]  (len(bases) == 1 shares the base, e.g. ScalarMultiplicationBase).
func G1ScalarMultiplicationBatch(bases []bn254.G1Affine, s []fr.Element) ([]bn254.G1Affine, error) {
	defer pin()()
	if len(s) == 0 {
		return nil, nil
	}
	if len(bases) != 1 && len(bases) != len(s) {
		return nil, errSizes
	}
	k := frBytes(s)
	out := make([]bn254.G1Affine, len(s))
	rc := C.gpbc_g1_scalar_mul_batch(unsafe.Pointer(unsafe.SliceData(bases)), C.size_t(len(bases)),
		unsafe.Pointer(unsafe.SliceData(k)), C.size_t(len(s)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// G2ScalarMultiplicationBatch: the same over G2.
func G2ScalarMultiplicationBatch(bases []bn254.G2Affine, s []fr.Element) ([]bn254.G2Affine, error) {
	defer pin()()
	if len(s) == 0 {
		return nil, nil
	}
	if len(bases) != 1 && len(bases) != len(s) {
		return nil, errSizes
	}
	k := frBytes(s)
	out := make([]bn254.G2Affine, len(s))
	rc := C.gpbc_g2_scalar_mul_batch(unsafe.Pointer(unsafe.SliceData(bases)), C.size_t(len(bases)),
		unsafe.Pointer(unsafe.SliceData(k)), C.size_t(len(s)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// G1AddBatch: out[i] = a[i] + b[i] (or + b[0] when len(b) == 1) — loops of (*bn254.G1Affine).Add between batched steps
// (dabe/lw11_dabe.go:100,157, cpabe/waters11/waters11_cpabe.go:226, bibe/afp25_bibe/afp25_bibe.go:216,252, ...).  out may be a
// (or b when len(b) == len(a)); nil allocates.  A single Add or Neg stays with gnark: it costs less on the host than a launch.
func G1AddBatch(out, a, b []bn254.G1Affine) ([]bn254.G1Affine, error) {
	return g1GroupOp(false, out, a, b)
}

// G1SubBatch: out[i] = a[i] - b[i] (or - b[0]) — (*bn254.G1Affine).Sub.
func G1SubBatch(out, a, b []bn254.G1Affine) ([]bn254.G1Affine, error) {
	return g1GroupOp(true, out, a, b)
}

// G1DoubleBatch: out[i] = 2 a[i] — (*bn254.G1Affine).Double.
func G1DoubleBatch(out, a []bn254.G1Affine) ([]bn254.G1Affine, error) {
	defer pin()()
	if len(a) == 0 {
		return out, nil
	}
	if out == nil {
		out = make([]bn254.G1Affine, len(a))
	}
	if len(out) != len(a) {
		return nil, errSizes
	}
	rc := C.gpbc_g1_double_batch(unsafe.Pointer(unsafe.SliceData(a)), C.size_t(len(a)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// G2AddBatch: out[i] = a[i] + b[i] (or + b[0]) — (*bn254.G2Affine).Add: BSW07 key components D_j = [r]g2 + [r_j]H(j)
// (cpabe/bsw07/bsw07_cpabe.go:104,119), ZSS04 verification [H(m)]g2 + pk (signature/zss04_signature/zss04_signature.go:327).
func G2AddBatch(out, a, b []bn254.G2Affine) ([]bn254.G2Affine, error) {
	return g2GroupOp(false, out, a, b)
}

// G2SubBatch: out[i] = a[i] - b[i] (or - b[0]) — (*bn254.G2Affine).Sub.
func G2SubBatch(out, a, b []bn254.G2Affine) ([]bn254.G2Affine, error) {
	return g2GroupOp(true, out, a, b)
}

// G2DoubleBatch: out[i] = 2 a[i] — (*bn254.G2Affine).Double.
func G2DoubleBatch(out, a []bn254.G2Affine) ([]bn254.G2Affine, error) {
	defer pin()()
	if len(a) == 0 {
		return out, nil
	}
	if out == nil {
		out = make([]bn254.G2Affine, len(a))
	}
	if len(out) != len(a) {
		return nil, errSizes
	}
	rc := C.gpbc_g2_double_batch(unsafe.Pointer(unsafe.SliceData(a)), C.size_t(len(a)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// Scalar-field batches: []fr.Element in, []fr.Element out.  Go holds an fr.Element as four Montgomery words (R = 2^256); the engine
// computes on the ABI's scalar format, so a batch goes through gpbc_fr_from_mont_batch once on the way in and gpbc_fr_to_mont_batch
// once on the way out — on the device, inside the same call sequence; no BigInt round trip per element.
const (
	frAdd = iota
	frSub
	frMul
	frNeg
	frInverse
)

// frPlain: the elements' words -> plain 32-byte scalars (what every `scalars` argument of the engine takes)
func frPlain(s []fr.Element) ([][32]byte, error) {
	k := make([][32]byte, len(s))
	if len(s) == 0 {
		return k, nil
	}
	rc := C.gpbc_fr_from_mont_batch(unsafe.Pointer(unsafe.SliceData(s)), C.size_t(len(s)), unsafe.Pointer(unsafe.SliceData(k)))
	return k, status(rc)
}

// frElements: plain scalars -> fr.Element words, into out
func frElements(k [][32]byte, out []fr.Element) error {
	if len(k) == 0 {
		return nil
	}
	return status(C.gpbc_fr_to_mont_batch(unsafe.Pointer(unsafe.SliceData(k)), C.size_t(len(k)), unsafe.Pointer(unsafe.SliceData(out))))
}

func frOp(op int, out, a, b []fr.Element) ([]fr.Element, error) {
	defer pin()()
	if len(a) == 0 {
		return out, nil
	}
	if out == nil {
		out = make([]fr.Element, len(a))
	}
	binary := op == frAdd || op == frSub || op == frMul
	if len(out) != len(a) || (binary && len(b) != 1 && len(b) != len(a)) {
		return nil, errSizes
	}
	ka, err := frPlain(a)
	if err != nil {
		return nil, err
	}
	pa, n := unsafe.Pointer(unsafe.SliceData(ka)), C.size_t(len(a))
	var rc C.int
	if binary {
		kb, err := frPlain(b)
		if err != nil {
			return nil, err
		}
		pb, nb := unsafe.Pointer(unsafe.SliceData(kb)), C.size_t(len(b))
		switch op {
		case frAdd:
			rc = C.gpbc_fr_add_batch(pa, pb, nb, n, pa)
		case frSub:
			rc = C.gpbc_fr_sub_batch(pa, pb, nb, n, pa)
		default:
			rc = C.gpbc_fr_mul_batch(pa, pb, nb, n, pa)
		}
	} else if op == frNeg {
		rc = C.gpbc_fr_neg_batch(pa, n, pa)
	} else {
		rc = C.gpbc_fr_inverse_batch(pa, n, pa)
	}
	if err := status(rc); err != nil {
		return nil, err
	}
	return out, frElements(ka, out)
}

// FrAddBatch / FrSubBatch / FrMulBatch: out[i] = a[i] OP b[i] (or b[0] when len(b) == 1) — loops of fr.Element.Add / Sub / Mul.
// out may be a or b; nil allocates.  A single operation stays with gnark: it costs nanoseconds on the host.
func FrAddBatch(out, a, b []fr.Element) ([]fr.Element, error) { return frOp(frAdd, out, a, b) }
func FrSubBatch(out, a, b []fr.Element) ([]fr.Element, error) { return frOp(frSub, out, a, b) }
func FrMulBatch(out, a, b []fr.Element) ([]fr.Element, error) { return frOp(frMul, out, a, b) }

// FrNegBatch: out[i] = -a[i].
func FrNegBatch(out, a []fr.Element) ([]fr.Element, error) { return frOp(frNeg, out, a, nil) }

// FrInverseBatch: out[i] = 1 / a[i], 0 for 0 as fr.Element.Inverse — the exponents 1 / (H(m) + x) of ZSS04 / BB04 signing
// (signature/zss04_signature/zss04_signature.go:249-252, signature/bb04_signature/bb04_signature.go:233) for a batch of messages.
func FrInverseBatch(out, a []fr.Element) ([]fr.Element, error) { return frOp(frInverse, out, a, nil) }

// FrPolyFromRoots: k polynomials prod_i (X - roots[j*B + i]), k x (B + 1) coefficients, constant term first —
// computePolynomialCoeffs (bibe/afp25_bibe/afp25_bibe_utils.go:14-43) for k batches at once.
func FrPolyFromRoots(roots []fr.Element, B int) ([]fr.Element, error) {
	defer pin()()
	if B < 1 || len(roots) == 0 || len(roots)%B != 0 {
		return nil, errSizes
	}
	k := len(roots) / B
	kr, err := frPlain(roots)
	if err != nil {
		return nil, err
	}
	kc := make([][32]byte, k*(B+1))
	rc := C.gpbc_fr_poly_from_roots(unsafe.Pointer(unsafe.SliceData(kr)), C.size_t(B), C.size_t(k), unsafe.Pointer(unsafe.SliceData(kc)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]fr.Element, len(kc))
	return out, frElements(kc, out)
}

// FrPolyQuotients: row j*B + i of the result holds the B coefficients of coeffs[j](X) / (X - points[j*B + i]) and stride - B zeros;
// ok[j*B + i] is false (and the row zero) where the point is not a root — the "identity not found" of the reference's Decrypt
// (bibe/afp25_bibe/afp25_bibe.go:369-418).
func FrPolyQuotients(coeffs, points []fr.Element, B, stride int) ([]fr.Element, []bool, error) {
	defer pin()()
	if B < 1 || stride < B || len(points) == 0 || len(points)%B != 0 || len(coeffs) != len(points)/B*(B+1) {
		return nil, nil, errSizes
	}
	k := len(points) / B
	kc, err := frPlain(coeffs)
	if err != nil {
		return nil, nil, err
	}
	kp, err := frPlain(points)
	if err != nil {
		return nil, nil, err
	}
	kq := make([][32]byte, len(points)*stride)
	okb := make([]byte, len(points))
	rc := C.gpbc_fr_poly_quotients(unsafe.Pointer(unsafe.SliceData(kc)), unsafe.Pointer(unsafe.SliceData(kp)), C.size_t(B), C.size_t(k), C.size_t(stride),
		unsafe.Pointer(unsafe.SliceData(kq)), (*C.uint8_t)(unsafe.SliceData(okb)))
	if err := status(rc); err != nil {
		return nil, nil, err
	}
	out := make([]fr.Element, len(kq))
	ok := make([]bool, len(okb))
	for i, b := range okb {
		ok[i] = b != 0
	}
	return out, ok, frElements(kq, out)
}

// FrLagrangeBasis: out[j*m + t] = prod over the elements s of set row j with s != node t of row j of (x[j] - s) / (node - s) —
// utils.ComputeLagrangeBasis for k rows whose node sets differ (fibe/sw05_fibe_common.go:316, fibe/sw05_fibe_large_universe.go:277 over
// S = FindCommonAttributes(...); computeT, sw05_fibe_large_universe.go:302-325).  set: one row of B elements or k rows; nodes: nil =
// the set's own elements, else one row of m or k rows; x: nil = evaluate at 0, else one element or k.
func FrLagrangeBasis(set []fr.Element, B int, nodes []fr.Element, m int, x []fr.Element) ([]fr.Element, error) {
	defer pin()()
	if B < 1 || len(set) == 0 || len(set)%B != 0 {
		return nil, errSizes
	}
	ns := len(set) / B
	nn := ns
	if nodes == nil {
		m = B
	} else if m < 1 || len(nodes) == 0 || len(nodes)%m != 0 {
		return nil, errSizes
	} else {
		nn = len(nodes) / m
	}
	nx := len(x)
	k := ns
	if nn > k {
		k = nn
	}
	if nx > k {
		k = nx
	}
	if (ns != 1 && ns != k) || (nn != 1 && nn != k) || (nx > 1 && nx != k) {
		return nil, errSizes
	}
	ks, err := frPlain(set)
	if err != nil {
		return nil, err
	}
	var pn, px unsafe.Pointer
	if nodes != nil {
		kn, err := frPlain(nodes)
		if err != nil {
			return nil, err
		}
		pn = unsafe.Pointer(unsafe.SliceData(kn))
	}
	if nx > 0 {
		kx, err := frPlain(x)
		if err != nil {
			return nil, err
		}
		px = unsafe.Pointer(unsafe.SliceData(kx))
	}
	ko := make([][32]byte, k*m)
	rc := C.gpbc_fr_lagrange_basis(unsafe.Pointer(unsafe.SliceData(ks)), C.size_t(ns), C.size_t(B), pn, C.size_t(nn), C.size_t(m), px, C.size_t(nx), C.size_t(k),
		unsafe.Pointer(unsafe.SliceData(ko)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]fr.Element, len(ko))
	return out, frElements(ko, out)
}

// FrPolyEval: out[j*m + t] = sum_i coeffs[j*d + i] points[j*m + t]^i — utils.ComputePolynomialValue over the coefficients of
// utils.GenerateRandomPolynomial for k rows (fibe/sw05_fibe_common.go:205-210, fibe/sw05_fibe_large_universe.go:153-167).  coeffs: one row
// of d elements (lowest degree first) or k rows; points: one row of m or k rows.
func FrPolyEval(coeffs []fr.Element, d int, points []fr.Element, m int) ([]fr.Element, error) {
	defer pin()()
	if d < 1 || len(coeffs) == 0 || len(coeffs)%d != 0 || m < 1 || len(points) == 0 || len(points)%m != 0 {
		return nil, errSizes
	}
	nc, np := len(coeffs)/d, len(points)/m
	k := nc
	if np > k {
		k = np
	}
	if (nc != 1 && nc != k) || (np != 1 && np != k) {
		return nil, errSizes
	}
	kc, err := frPlain(coeffs)
	if err != nil {
		return nil, err
	}
	kp, err := frPlain(points)
	if err != nil {
		return nil, err
	}
	ko := make([][32]byte, k*m)
	rc := C.gpbc_fr_poly_eval(unsafe.Pointer(unsafe.SliceData(kc)), C.size_t(nc), C.size_t(d), unsafe.Pointer(unsafe.SliceData(kp)), C.size_t(np), C.size_t(m), C.size_t(k),
		unsafe.Pointer(unsafe.SliceData(ko)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]fr.Element, len(ko))
	return out, frElements(ko, out)
}

// ShareNode is one node of a threshold tree in depth-first preorder: Parent is the index of its parent (ShareRoot for node 0),
// Threshold 0 marks a leaf, otherwise the gate's k of k-of-n.
type ShareNode struct{ Parent, Threshold uint32 }

const ShareRoot = 0xffffffff

// ShareTree is a threshold tree uploaded once; Share is AccessTreeNode.ShareSecret (access/tree/access_tree_node.go:58-75) for k secrets
// in one launch: coeffs holds Coeffs() elements per secret, gate by gate in the order ShareSecret draws them, and the result Leaves()
// shares per secret in leaf order (leaf id y of GenerateLeafID is column y - 1).
type ShareTree struct{ h *C.gpbc_share_tree }

func NewShareTree(nodes []ShareNode) (*ShareTree, error) {
	defer pin()()
	t := &ShareTree{}
	rc := C.gpbc_share_tree_create((*C.gpbc_share_node)(unsafe.Pointer(unsafe.SliceData(nodes))), C.size_t(len(nodes)), &t.h)
	if err := status(rc); err != nil {
		return nil, err
	}
	return t, nil
}
func (t *ShareTree) Leaves() int { return int(C.gpbc_share_tree_leaves(t.h)) }
func (t *ShareTree) Coeffs() int { return int(C.gpbc_share_tree_coeffs(t.h)) }
func (t *ShareTree) Close() {
	C.gpbc_share_tree_destroy(t.h)
	t.h = nil
}
func (t *ShareTree) Share(secrets, coeffs []fr.Element) ([]fr.Element, error) {
	defer pin()()
	if len(coeffs) != len(secrets)*t.Coeffs() {
		return nil, errSizes
	}
	ks, err := frPlain(secrets)
	if err != nil {
		return nil, err
	}
	var pc unsafe.Pointer
	if len(coeffs) > 0 {
		kc, err := frPlain(coeffs)
		if err != nil {
			return nil, err
		}
		pc = unsafe.Pointer(unsafe.SliceData(kc))
	}
	ko := make([][32]byte, len(secrets)*t.Leaves())
	rc := C.gpbc_fr_share_tree(t.h, unsafe.Pointer(unsafe.SliceData(ks)), pc, C.size_t(len(secrets)), unsafe.Pointer(unsafe.SliceData(ko)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]fr.Element, len(ko))
	return out, frElements(ko, out)
}

// FrLsssWeights: for k systems the weights w with sum_x w[x] M[x] = (1, 0, ..., 0) over the rows the key holds —
// FindLinearCombinationWeight (access/lsss/lewko_waters_lsss_matrix.go:167-429) where the matrix differs per item, as in the Decrypt of
// cpabe/waters11 (waters11_cpabe.go:254) over a batch of ciphertexts.  matrix: one rows x cols matrix or k of them, row-major; held:
// k x rows bytes, non-zero = held.  Returns k x rows weights (0 for a row that is not used) and k ok bytes (0: not satisfied, the row
// of weights is zero).  The used rows are the greedy first basis of the held rows, see include/gpbc_bn254.h.
func FrLsssWeights(matrix []fr.Element, rows, cols int, held []byte) ([]fr.Element, []byte, error) {
	defer pin()()
	if rows < 1 || cols < 1 || len(matrix) == 0 || len(matrix)%(rows*cols) != 0 || len(held)%rows != 0 {
		return nil, nil, errSizes
	}
	nm := len(matrix) / (rows * cols)
	k := len(held) / rows
	if nm != 1 && nm != k {
		return nil, nil, errSizes
	}
	if k == 0 {
		return nil, nil, nil
	}
	km, err := frPlain(matrix)
	if err != nil {
		return nil, nil, err
	}
	kw := make([][32]byte, k*rows)
	ok := make([]byte, k)
	rc := C.gpbc_fr_lsss_weights(unsafe.Pointer(unsafe.SliceData(km)), C.size_t(nm), C.size_t(rows), C.size_t(cols), (*C.uint8_t)(unsafe.SliceData(held)), C.size_t(k),
		unsafe.Pointer(unsafe.SliceData(kw)), (*C.uint8_t)(unsafe.SliceData(ok)))
	if err := status(rc); err != nil {
		return nil, nil, err
	}
	out := make([]fr.Element, len(kw))
	return out, ok, frElements(kw, out)
}

// FrLsssShares: the shares lambda_x = M_x . v of LewkoWatersLsssMatrix.ComputeVector for k vectors in one launch
// (include/gpbc_bn254_indexed.h): matrix holds one rows x cols matrix (shared by the k vectors) or k of them, vectors k x cols
// elements.  Returns k x rows elements.
func FrLsssShares(matrix []fr.Element, rows, cols int, vectors []fr.Element) ([]fr.Element, error) {
	defer pin()()
	if rows < 1 || cols < 1 || len(matrix) == 0 || len(matrix)%(rows*cols) != 0 || len(vectors)%cols != 0 {
		return nil, errSizes
	}
	nm := len(matrix) / (rows * cols)
	k := len(vectors) / cols
	if k == 0 {
		return nil, nil
	}
	if nm != 1 && nm != k {
		return nil, errSizes
	}
	km, err := frPlain(matrix)
	if err != nil {
		return nil, err
	}
	kv, err := frPlain(vectors)
	if err != nil {
		return nil, err
	}
	ko := make([][32]byte, k*rows)
	rc := C.gpbc_fr_lsss_shares(unsafe.Pointer(unsafe.SliceData(km)), C.size_t(nm), C.size_t(rows), C.size_t(cols), unsafe.Pointer(unsafe.SliceData(kv)), C.size_t(k),
		unsafe.Pointer(unsafe.SliceData(ko)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]fr.Element, len(ko))
	return out, frElements(ko, out)
}

// FrFindCommon: utils.FindCommonAttributes for k lists of a elements in one launch (include/gpbc_bn254_select.h): sets holds one set
// of m elements (shared by the k lists) or k of them.  Per list and slot s < d: the position of the s-th kept element in the set (its
// first occurrence) and in the list, and the element; ok[j] == 0, and zero rows, where fewer than d are common.
func FrFindCommon(sets []fr.Element, m int, lists []fr.Element, a, d int) (setPos, listPos []uint32, common []fr.Element, ok []uint8, err error) {
	defer pin()()
	if m < 1 || a < 1 || d < 1 || len(sets) == 0 || len(sets)%m != 0 || len(lists)%a != 0 {
		return nil, nil, nil, nil, errSizes
	}
	ns := len(sets) / m
	k := len(lists) / a
	if k == 0 {
		return nil, nil, nil, nil, nil
	}
	if ns != 1 && ns != k {
		return nil, nil, nil, nil, errSizes
	}
	ks, err := frPlain(sets)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	kl, err := frPlain(lists)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	setPos, listPos, ok = make([]uint32, k*d), make([]uint32, k*d), make([]uint8, k)
	kc := make([][32]byte, k*d)
	rc := C.gpbc_fr_find_common(unsafe.Pointer(unsafe.SliceData(ks)), C.size_t(ns), C.size_t(m), unsafe.Pointer(unsafe.SliceData(kl)), C.size_t(a), C.size_t(d), C.size_t(k),
		(*C.uint32_t)(unsafe.SliceData(setPos)), (*C.uint32_t)(unsafe.SliceData(listPos)), unsafe.Pointer(unsafe.SliceData(kc)), (*C.uint8_t)(unsafe.SliceData(ok)))
	if err := status(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	common = make([]fr.Element, len(kc))
	return setPos, listPos, common, ok, frElements(kc, common)
}

// FrDotSegments: out[s] = sum_{i in [segOff[s], segOff[s+1])} a[i] * b[i] (include/gpbc_bn254_verify.h) — the scalar sums of a batch
// verifier (sum rho_i per group of signatures) and of the planners' checks (sum w_x lambda_x = s).  b holds one element per a, or ONE
// list for segments of one length, or is nil for the plain sums.  segOff: len(out) + 1 non-decreasing offsets from 0 to len(a).
func FrDotSegments(a, b []fr.Element, segOff []uint64) ([]fr.Element, error) {
	defer pin()()
	if len(segOff) < 1 || segOff[len(segOff)-1] != uint64(len(a)) {
		return nil, errSizes
	}
	nSeg := len(segOff) - 1
	if nSeg == 0 {
		return nil, nil
	}
	ka, err := frPlain(a)
	if err != nil {
		return nil, err
	}
	var kb [][32]byte
	if b != nil {
		if kb, err = frPlain(b); err != nil {
			return nil, err
		}
	}
	ko := make([][32]byte, nSeg)
	rc := C.gpbc_fr_dot_segments(unsafe.Pointer(unsafe.SliceData(ka)), unsafe.Pointer(unsafe.SliceData(kb)), C.size_t(len(kb)), (*C.uint64_t)(unsafe.SliceData(segOff)),
		C.size_t(nSeg), unsafe.Pointer(unsafe.SliceData(ko)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]fr.Element, nSeg)
	return out, frElements(ko, out)
}

// GTEqual: ok[i] = a[i].Equal(&b[i]), or a[i].Equal(&b[0]) for a single b, for n elements in one launch (include/gpbc_bn254_verify.h):
// pairLeft.Equal(&pp.eG1G2) of signature/zss04_signature/zss04_signature.go:337 and signature/bb04_signature/bb04_signature.go:292.
func GTEqual(a, b []bn254.GT) ([]bool, error) {
	defer pin()()
	if len(b) != len(a) && len(b) != 1 {
		return nil, errSizes
	}
	if len(a) == 0 {
		return nil, nil
	}
	ok := make([]uint8, len(a))
	rc := C.gpbc_gt_equal(unsafe.Pointer(unsafe.SliceData(a)), unsafe.Pointer(unsafe.SliceData(b)), C.size_t(len(b)), C.size_t(len(a)), (*C.uint8_t)(unsafe.SliceData(ok)))
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([]bool, len(a))
	for i, v := range ok {
		out[i] = v != 0
	}
	return out, nil
}

// g1GroupOp: Add (sub == false) or Sub over the batch (cgo cannot take a C function as a value, hence the flag)
func g1GroupOp(sub bool, out, a, b []bn254.G1Affine) ([]bn254.G1Affine, error) {
	defer pin()()
	if len(a) == 0 {
		return out, nil
	}
	if out == nil {
		out = make([]bn254.G1Affine, len(a))
	}
	if (len(b) != 1 && len(b) != len(a)) || len(out) != len(a) {
		return nil, errSizes
	}
	pa, pb, po := unsafe.Pointer(unsafe.SliceData(a)), unsafe.Pointer(unsafe.SliceData(b)), unsafe.Pointer(unsafe.SliceData(out))
	var rc C.int
	if sub {
		rc = C.gpbc_g1_sub_batch(pa, pb, C.size_t(len(b)), C.size_t(len(a)), po)
	} else {
		rc = C.gpbc_g1_add_batch(pa, pb, C.size_t(len(b)), C.size_t(len(a)), po)
	}
	return out, status(rc)
}

// g2GroupOp: Add (sub == false) or Sub over the batch (cgo cannot take a C function as a value, hence the flag)
func g2GroupOp(sub bool, out, a, b []bn254.G2Affine) ([]bn254.G2Affine, error) {
	defer pin()()
	if len(a) == 0 {
		return out, nil
	}
	if out == nil {
		out = make([]bn254.G2Affine, len(a))
	}
	if (len(b) != 1 && len(b) != len(a)) || len(out) != len(a) {
		return nil, errSizes
	}
	pa, pb, po := unsafe.Pointer(unsafe.SliceData(a)), unsafe.Pointer(unsafe.SliceData(b)), unsafe.Pointer(unsafe.SliceData(out))
	var rc C.int
	if sub {
		rc = C.gpbc_g2_sub_batch(pa, pb, C.size_t(len(b)), C.size_t(len(a)), po)
	} else {
		rc = C.gpbc_g2_add_batch(pa, pb, C.size_t(len(b)), C.size_t(len(a)), po)
	}
	return out, status(rc)
}

// G1ScalarMulSum = sum_i [s[i]] bases[i]: the verifier's side of BLS aggregate verification with random linear
// combination (a loop of ScalarMultiplication + Add in the reference's style, gka/agka09/asbb.go:193-220), sharded over
// all bound GPUs with the partial sums combined inside the library.
func G1ScalarMulSum(bases []bn254.G1Affine, s []fr.Element) (bn254.G1Affine, error) {
	defer pin()()
	var out bn254.G1Affine
	if len(bases) != len(s) {
		return out, errSizes
	}
	if len(s) == 0 {
		return out, nil
	}
	k := frBytes(s)
	rc := C.gpbc_g1_scalar_mul_sum(unsafe.Pointer(unsafe.SliceData(bases)), unsafe.Pointer(unsafe.SliceData(k)), C.size_t(len(s)), unsafe.Pointer(&out))
	return out, status(rc)
}

// G2ScalarMulSum: the same over G2.
func G2ScalarMulSum(bases []bn254.G2Affine, s []fr.Element) (bn254.G2Affine, error) {
	defer pin()()
	var out bn254.G2Affine
	if len(bases) != len(s) {
		return out, errSizes
	}
	if len(s) == 0 {
		return out, nil
	}
	k := frBytes(s)
	rc := C.gpbc_g2_scalar_mul_sum(unsafe.Pointer(unsafe.SliceData(bases)), unsafe.Pointer(unsafe.SliceData(k)), C.size_t(len(s)), unsafe.Pointer(&out))
	return out, status(rc)
}

// gtExp256: z = x^e for one 32-byte little-endian exponent.
func gtExp256(x *bn254.GT, e *[32]byte) bn254.GT {
	var z bn254.GT
	must(C.gpbc_gt_exp_batch(unsafe.Pointer(x), unsafe.Pointer(&e[0]), 1, unsafe.Pointer(&z)))
	return z
}

// GTExp replaces new(bn254.GT).Exp(x, k) (access/tree/access_tree_node.go:123,156; bibe/afp25_bibe/afp25_bibe.go:258-259).
// Like gnark it takes ANY big.Int and does not reduce it (x need not lie in the order-r subgroup: the reference's
// SetRandom messages do not): a negative k inverts x first; an exponent wider than the kernel's 256 bits is evaluated in
// 256-bit digits, x^k = prod_i (x^(2^(256 i)))^(k_i).  The reference's call sites pass values below r: one digit.
func GTExp(z *bn254.GT, x bn254.GT, k *big.Int) *bn254.GT {
	defer pin()()
	var abs big.Int
	abs.Abs(k)
	base := x
	if k.Sign() < 0 {
		var inv bn254.GT
		must(C.gpbc_gt_inverse_batch(unsafe.Pointer(&x), 1, unsafe.Pointer(&inv)))
		base = inv
	}
	var acc bn254.GT
	acc.SetOne()
	mask := new(big.Int).Sub(new(big.Int).Lsh(big.NewInt(1), 256), big.NewInt(1))
	var two255, two [32]byte
	two255[31] = 0x80
	two[0] = 2
	for first := true; ; first = false {
		var digit big.Int
		digit.And(&abs, mask)
		var e [32]byte
		b := digit.Bytes() // at most 32 bytes
		for i := range b {
			e[len(b)-1-i] = b[i]
		}
		t := gtExp256(&base, &e)
		if first {
			acc = t
		} else {
			must(C.gpbc_gt_mul_batch(unsafe.Pointer(&acc), unsafe.Pointer(&t), 1, unsafe.Pointer(&acc)))
		}
		abs.Rsh(&abs, 256)
		if abs.Sign() == 0 {
			break
		}
		h := gtExp256(&base, &two255) // base^(2^256) = (base^(2^255))^2
		base = gtExp256(&h, &two)
	}
	*z = acc
	return z
}

// GTMultiExp: z = prod_i xs[i]^ks[i] in ONE call — the loop `res.Mul(res, tmp.Exp(c, w))` of dabe/lw11_dabe.go:180-196 and of the
// threshold gates (access/tree/access_tree_node.go:123,156) with the squarings shared among the factors.  Exponents as in GTExp:
// any big.Int, not reduced; a negative one inverts its base first; one wider than 256 bits contributes one factor per 256-bit
// digit, x^k = prod_j (x^(2^(256 j)))^(k_j).  No factors: one.
func GTMultiExp(z *bn254.GT, xs []bn254.GT, ks []*big.Int) (*bn254.GT, error) {
	defer pin()()
	if len(xs) != len(ks) {
		return z, errSizes
	}
	mask := new(big.Int).Sub(new(big.Int).Lsh(big.NewInt(1), 256), big.NewInt(1))
	var two255, two [32]byte
	two255[31] = 0x80
	two[0] = 2
	bases := make([]bn254.GT, 0, len(xs))
	exps := make([]byte, 0, 32*len(xs))
	for i := range xs {
		var abs big.Int
		abs.Abs(ks[i])
		base := xs[i]
		if ks[i].Sign() < 0 {
			var inv bn254.GT
			must(C.gpbc_gt_inverse_batch(unsafe.Pointer(&xs[i]), 1, unsafe.Pointer(&inv)))
			base = inv
		}
		for {
			var digit big.Int
			digit.And(&abs, mask)
			var e [32]byte
			b := digit.Bytes() // at most 32 bytes
			for j := range b {
				e[len(b)-1-j] = b[j]
			}
			bases = append(bases, base)
			exps = append(exps, e[:]...)
			abs.Rsh(&abs, 256)
			if abs.Sign() == 0 {
				break
			}
			h := gtExp256(&base, &two255) // base^(2^256) = (base^(2^255))^2
			base = gtExp256(&h, &two)
		}
	}
	var out bn254.GT
	out.SetOne()
	if len(bases) > 0 {
		seg := [2]C.uint64_t{0, C.uint64_t(len(bases))}
		rc := C.gpbc_gt_multi_exp(unsafe.Pointer(unsafe.SliceData(bases)), unsafe.Pointer(unsafe.SliceData(exps)), C.size_t(len(bases)), &seg[0], 1, unsafe.Pointer(&out))
		if err := status(rc); err != nil {
			return z, err
		}
	}
	*z = out
	return z, nil
}

// GTProd: z = prod_i xs[i], the chain `aggregateA.Mul(&aggregateA, &pk.A)` of gka/agka09/asbb.go:193-207 as one call (the GT
// sibling of G1Sum).  No factors: one.
func GTProd(z *bn254.GT, xs []bn254.GT) (*bn254.GT, error) {
	defer pin()()
	var out bn254.GT
	out.SetOne()
	if len(xs) > 0 {
		seg := [2]C.uint64_t{0, C.uint64_t(len(xs))}
		rc := C.gpbc_gt_multi_exp(unsafe.Pointer(unsafe.SliceData(xs)), nil, 0, &seg[0], 1, unsafe.Pointer(&out))
		if err := status(rc); err != nil {
			return z, err
		}
	}
	*z = out
	return z, nil
}

// GTMul, GTDiv, GTInverse replace new(bn254.GT).Mul(x, y) / Div(x, y) / Inverse(x) with gnark's signatures
// (access/tree/access_tree_node.go:114,157; cpabe/bsw07/bsw07_cpabe.go:189-190): z may alias an operand.
func GTMul(z, x, y *bn254.GT) *bn254.GT {
	defer pin()()
	var out bn254.GT
	must(C.gpbc_gt_mul_batch(unsafe.Pointer(x), unsafe.Pointer(y), 1, unsafe.Pointer(&out)))
	*z = out
	return z
}
func GTDiv(z, x, y *bn254.GT) *bn254.GT {
	defer pin()()
	var out bn254.GT
	must(C.gpbc_gt_div_batch(unsafe.Pointer(x), unsafe.Pointer(y), 1, unsafe.Pointer(&out)))
	*z = out
	return z
}
func GTInverse(z, x *bn254.GT) *bn254.GT {
	defer pin()()
	var out bn254.GT
	must(C.gpbc_gt_inverse_batch(unsafe.Pointer(x), 1, unsafe.Pointer(&out)))
	*z = out
	return z
}

// The batched forms: one element per index.
func GTMulBatch(a, b []bn254.GT) ([]bn254.GT, error) {
	defer pin()()
	if len(a) != len(b) {
		return nil, errSizes
	}
	out := make([]bn254.GT, len(a))
	if len(a) == 0 {
		return out, nil
	}
	rc := C.gpbc_gt_mul_batch(unsafe.Pointer(unsafe.SliceData(a)), unsafe.Pointer(unsafe.SliceData(b)), C.size_t(len(a)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}
func GTDivBatch(a, b []bn254.GT) ([]bn254.GT, error) {
	defer pin()()
	if len(a) != len(b) {
		return nil, errSizes
	}
	out := make([]bn254.GT, len(a))
	if len(a) == 0 {
		return out, nil
	}
	rc := C.gpbc_gt_div_batch(unsafe.Pointer(unsafe.SliceData(a)), unsafe.Pointer(unsafe.SliceData(b)), C.size_t(len(a)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// MarshalG1Batch / UnmarshalG1Batch replace element.Marshal() / g1.Unmarshal(data)
// (serialization/serialization_curve.go:5-7,17-21) n elements per call.  Unlike the reference, the decode error is
// returned per element, not dropped.
func MarshalG1Batch(pts []bn254.G1Affine, compressed bool) []byte {
	defer pin()()
	w, c := 64, C.int(0)
	if compressed {
		w, c = 32, 1
	}
	out := make([]byte, w*len(pts))
	if len(pts) > 0 {
		must(C.gpbc_g1_marshal_batch(unsafe.Pointer(unsafe.SliceData(pts)), C.size_t(len(pts)), c, unsafe.Pointer(unsafe.SliceData(out))))
	}
	return out
}
func UnmarshalG1Batch(data []byte, elemBytes int) ([]bn254.G1Affine, []bool, error) {
	defer pin()()
	if elemBytes != 32 && elemBytes != 64 {
		return nil, nil, errors.New("G1 element size must be 32 or 64")
	}
	n := len(data) / elemBytes
	out, ok8, ok := make([]bn254.G1Affine, n), make([]uint8, n), make([]bool, n)
	if n == 0 {
		return out, ok, nil
	}
	rc := C.gpbc_g1_unmarshal_batch(unsafe.Pointer(unsafe.SliceData(data)), C.size_t(elemBytes), C.size_t(n),
		unsafe.Pointer(unsafe.SliceData(out)), (*C.uint8_t)(unsafe.SliceData(ok8)))
	for i := range ok8 {
		ok[i] = ok8[i] == 1
	}
	return out, ok, status(rc)
}
func MarshalG2Batch(pts []bn254.G2Affine, compressed bool) []byte {
	defer pin()()
	w, c := 128, C.int(0)
	if compressed {
		w, c = 64, 1
	}
	out := make([]byte, w*len(pts))
	if len(pts) > 0 {
		must(C.gpbc_g2_marshal_batch(unsafe.Pointer(unsafe.SliceData(pts)), C.size_t(len(pts)), c, unsafe.Pointer(unsafe.SliceData(out))))
	}
	return out
}
func UnmarshalG2Batch(data []byte, elemBytes int) ([]bn254.G2Affine, []bool, error) {
	defer pin()()
	if elemBytes != 64 && elemBytes != 128 {
		return nil, nil, errors.New("G2 element size must be 64 or 128")
	}
	n := len(data) / elemBytes
	out, ok8, ok := make([]bn254.G2Affine, n), make([]uint8, n), make([]bool, n)
	if n == 0 {
		return out, ok, nil
	}
	rc := C.gpbc_g2_unmarshal_batch(unsafe.Pointer(unsafe.SliceData(data)), C.size_t(elemBytes), C.size_t(n),
		unsafe.Pointer(unsafe.SliceData(out)), (*C.uint8_t)(unsafe.SliceData(ok8)))
	for i := range ok8 {
		ok[i] = ok8[i] == 1
	}
	return out, ok, status(rc)
}
func MarshalGTBatch(gt []bn254.GT) []byte { // GT.Marshal() = GT.Bytes() (hash/hash_from_gt.go:5-8)
	defer pin()()
	out := make([]byte, 384*len(gt))
	if len(gt) > 0 {
		must(C.gpbc_gt_marshal_batch(unsafe.Pointer(unsafe.SliceData(gt)), C.size_t(len(gt)), unsafe.Pointer(unsafe.SliceData(out))))
	}
	return out
}

// UnmarshalG1, UnmarshalG2, UnmarshalGT replace (*G1Affine).Unmarshal(buf) / (*G2Affine).Unmarshal / (*GT).Unmarshal
// (serialization/serialization_curve.go:17-33, whose callers drop the error).  Like gnark they accept the compressed and the
// uncompressed form by the flag bits of the first byte and return an error for a short buffer, a coordinate >= p, a point off
// the curve or outside the subgroup; the receiver is then left zero.
var errShort = errors.New("short buffer")
var errInvalidEncoding = errors.New("invalid point encoding")

func UnmarshalG1(p *bn254.G1Affine, buf []byte) error {
	defer pin()()
	if len(buf) < 32 {
		return errShort
	}
	size := 64
	if buf[0]&0xC0 != 0 { // mCompressedSmallest, mCompressedLargest or mCompressedInfinity
		size = 32
	} else if len(buf) < 64 {
		return errShort
	}
	var ok C.uint8_t
	if err := status(C.gpbc_g1_unmarshal_batch(unsafe.Pointer(unsafe.SliceData(buf)), C.size_t(size), 1, unsafe.Pointer(p), &ok)); err != nil {
		return err
	}
	if ok != 1 {
		return errInvalidEncoding
	}
	return nil
}
func UnmarshalG2(p *bn254.G2Affine, buf []byte) error {
	defer pin()()
	if len(buf) < 64 {
		return errShort
	}
	size := 128
	if buf[0]&0xC0 != 0 {
		size = 64
	} else if len(buf) < 128 {
		return errShort
	}
	var ok C.uint8_t
	if err := status(C.gpbc_g2_unmarshal_batch(unsafe.Pointer(unsafe.SliceData(buf)), C.size_t(size), 1, unsafe.Pointer(p), &ok)); err != nil {
		return err
	}
	if ok != 1 {
		return errInvalidEncoding
	}
	return nil
}
func UnmarshalGT(z *bn254.GT, buf []byte) error {
	defer pin()()
	if len(buf) < 384 {
		return errShort
	}
	var ok C.uint8_t
	if err := status(C.gpbc_gt_unmarshal_batch(unsafe.Pointer(unsafe.SliceData(buf)), 1, unsafe.Pointer(z), &ok)); err != nil {
		return err
	}
	if ok != 1 {
		return errInvalidEncoding
	}
	return nil
}

// HashToG1 and HashToG2 replace bn254.HashToG1(msg, dst) / bn254.HashToG2(msg, dst) with gnark's signatures
// (hash/hash_to.go:114,170,205,272 — one call per string in the reference).
func HashToG1(msg, dst []byte) (bn254.G1Affine, error) {
	out, err := HashToG1Batch([][]byte{msg}, dst)
	if err != nil {
		return bn254.G1Affine{}, err
	}
	return out[0], nil
}
func HashToG2(msg, dst []byte) (bn254.G2Affine, error) {
	out, err := HashToG2Batch([][]byte{msg}, dst)
	if err != nil {
		return bn254.G2Affine{}, err
	}
	return out[0], nil
}

// HashToG1Batch replaces bn254.HashToG1(msg, dst) (hash/hash_to.go:113-119,169-175) for a batch: the engine hashes
// (expand_message_xmd with SHA-256, reduction to two field elements), maps both, adds.
func HashToG1Batch(msgs [][]byte, dst []byte) ([]bn254.G1Affine, error) {
	defer pin()()
	out := make([]bn254.G1Affine, len(msgs))
	if len(msgs) == 0 {
		return out, nil
	}
	if len(dst) > 255 {
		return nil, errors.New("invalid domain size (>255 bytes)") // what gnark's ExpandMsgXmd answers
	}
	data, off := flatten(msgs)
	rc := C.gpbc_hash_to_g1(unsafe.Pointer(unsafe.SliceData(data)), (*C.uint64_t)(unsafe.SliceData(off)), C.size_t(len(msgs)),
		dstPointer(dst), C.size_t(len(dst)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// HashG1GTGTToFr is h(u, v, w) of ibe/gentry06_ibe/gentry06_ibe.go:319-343 for n items: fr.SetBytes(SHA-256(u.Bytes() || v.Bytes() || w.Bytes())).
func HashG1GTGTToFr(u []bn254.G1Affine, v, w []bn254.GT) ([]fr.Element, error) {
	defer pin()()
	if len(u) != len(v) || len(u) != len(w) {
		return nil, errSizes
	}
	k, out := make([][32]byte, len(u)), make([]fr.Element, len(u))
	if len(u) == 0 {
		return out, nil
	}
	rc := C.gpbc_hash_g1_gt_gt_to_fr(unsafe.Pointer(unsafe.SliceData(u)), unsafe.Pointer(unsafe.SliceData(v)), unsafe.Pointer(unsafe.SliceData(w)),
		C.size_t(len(u)), unsafe.Pointer(unsafe.SliceData(k)))
	if err := status(rc); err != nil {
		return nil, err
	}
	return out, frElements(k, out)
}

// Sha256Batch is sha256.Sum256 per message (NewWaters05IBEIdentity, NewBB04IBEIdentity); Sha256ToFrBatch is fr.SetBytes of it.
func Sha256Batch(msgs [][]byte) ([][32]byte, error) {
	defer pin()()
	out := make([][32]byte, len(msgs))
	if len(msgs) == 0 {
		return out, nil
	}
	data, off := flatten(msgs)
	rc := C.gpbc_sha256_batch(unsafe.Pointer(unsafe.SliceData(data)), (*C.uint64_t)(unsafe.SliceData(off)), C.size_t(len(msgs)), 0, unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}
func Sha256ToFrBatch(msgs [][]byte) ([]fr.Element, error) {
	defer pin()()
	k, out := make([][32]byte, len(msgs)), make([]fr.Element, len(msgs))
	if len(msgs) == 0 {
		return out, nil
	}
	data, off := flatten(msgs)
	rc := C.gpbc_sha256_batch(unsafe.Pointer(unsafe.SliceData(data)), (*C.uint64_t)(unsafe.SliceData(off)), C.size_t(len(msgs)), 1, unsafe.Pointer(unsafe.SliceData(k)))
	if err := status(rc); err != nil {
		return nil, err
	}
	return out, frElements(k, out)
}

// MapToG1Batch is the group part alone for callers that hold gnark's fp.Hash(msg, dst, 2) output already: u has two
// elements per point, out[i] = MapToCurve1(u[2i]) + MapToCurve1(u[2i+1]).
func MapToG1Batch(u []fp.Element) ([]bn254.G1Affine, error) {
	defer pin()()
	if len(u)%2 != 0 {
		return nil, errors.New("two field elements per point")
	}
	out := make([]bn254.G1Affine, len(u)/2)
	if len(out) == 0 {
		return out, nil
	}
	rc := C.gpbc_g1_map_to_curve_batch(unsafe.Pointer(unsafe.SliceData(u)), C.size_t(len(out)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// HashToG2Batch replaces bn254.HashToG2 (hash/hash_to.go:204-210,271-277): four base-field elements per message,
// E2 j = elements 2j (A0) and 2j+1 (A1); hashing, both maps, addition and cofactor clearing in one call.
func HashToG2Batch(msgs [][]byte, dst []byte) ([]bn254.G2Affine, error) {
	defer pin()()
	out := make([]bn254.G2Affine, len(msgs))
	if len(msgs) == 0 {
		return out, nil
	}
	if len(dst) > 255 {
		return nil, errors.New("invalid domain size (>255 bytes)") // what gnark's ExpandMsgXmd answers
	}
	data, off := flatten(msgs)
	rc := C.gpbc_hash_to_g2(unsafe.Pointer(unsafe.SliceData(data)), (*C.uint64_t)(unsafe.SliceData(off)), C.size_t(len(msgs)),
		dstPointer(dst), C.size_t(len(dst)), unsafe.Pointer(unsafe.SliceData(out)))
	return out, status(rc)
}

// dstPointer: an empty domain-separation tag is legal (the library accepts dst == NULL with dst_len == 0, and so does this shim:
// unsafe.SliceData of an empty slice may be nil).
func dstPointer(dst []byte) unsafe.Pointer {
	if len(dst) == 0 {
		return nil
	}
	return unsafe.Pointer(unsafe.SliceData(dst))
}

// flatten lays the messages back to back with their n+1 byte offsets (the layout of gpbc_hash_to_*).
func flatten(msgs [][]byte) ([]byte, []uint64) {
	off := make([]uint64, len(msgs)+1)
	total := 0
	for i, m := range msgs {
		total += len(m)
		off[i+1] = uint64(total)
	}
	data := make([]byte, 0, total+1)
	for _, m := range msgs {
		data = append(data, m...)
	}
	if len(data) == 0 {
		data = append(data, 0) // SliceData of an empty slice may be nil
	}
	return data, off
}
