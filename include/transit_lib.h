/* transit_lib.h -- libtransit.so: the library interface of the reference `transit`
 * (the eight functions of transit/src/transit.c:14-22, which its SWIG module transit.i
 * wraps for retrieval drivers such as BART), with the same C prototypes, so that a C caller
 * written for the reference re-links with
 *
 *     cc driver.c -I include -L transit_amd/lib -ltransit -Wl,-rpath,<that lib directory>
 *
 * Per process there is ONE state, as in the reference: transit_init() loads a configuration
 * and keeps the line list, samplings and tables resident on the GPU; every run_transit() takes
 * one atmosphere and computes one spectrum.  The functions are not thread-safe: call them
 * from one thread at a time.
 *
 * The GPU is device 0 of those the process can see; choose it per process with
 * HIP_VISIBLE_DEVICES.  The library never changes the environment.
 *
 * Where it differs from the reference:
 *   - it never exits or aborts the process: a failure sets transit_status() / transit_error(),
 *     prints one line to stderr and leaves the state as described below;
 *   - the sizes passed in are honoured: get_waveno_arr() and run_transit() write exactly
 *     `waveno` / `transit_out_size` values (zeros past the number of samples);
 *   - a run_transit() that fails, or comes before transit_init(), fills its output with NaN;
 *   - transit_status() and transit_error() are additions.
 */
#ifndef TRANSIT_LIB_H
#define TRANSIT_LIB_H

#ifdef __cplusplus
extern "C" {
#endif

/* argv[0] is the program name, argv[1..argc) the reference's command line (e.g. "-c", "run.cfg").
 * Frees an earlier state first.  Builds and writes the opacity grid when --opacityfile names a
 * file that does not exist yet.  With --justOpacity the library stays initialised and
 * run_transit() computes nothing.  On failure nothing stays initialised.  --help / --version
 * print and leave nothing initialised, with status 0. */
void transit_init(int argc, char **argv);

/* number of wavenumber samples; 0 when not initialised */
int  get_no_samples(void);

/* the first min(waveno, samples) wavenumbers (cm-1), zeros after them; -1 everywhere when not
 * initialised */
void get_waveno_arr(double *waveno_arr, int waveno);

/* reference radius, cloud top (turns on the reference's grey cloud) and scattering of the
 * following runs; no effect (but a status) when not initialised */
void set_radius(double refradius);
void set_cloudtop(double cloudtop);
void set_scattering(int flag, double scattering);

/* One spectrum for the atmosphere re_input = [T(nlayer), q_0(nlayer), ..., q_{nmol-1}(nlayer)]
 * of transint values: writes min(transit_out_size, samples) values, zeros after them, and the
 * files the configuration names (spectrum, and toomuch, intensities, savefiles dumps, detail
 * and saveext files when asked for), as the reference does on every call. */
void run_transit(double *re_input, int transint, double *transit_out, int transit_out_size);

/* release everything transit_init() made; harmless when nothing is initialised */
void free_memory(void);

/* status of the last call above: 0 on success, else a negative trx_status of transit_hip.h */
int  transit_status(void);
/* its message; "" on success */
const char *transit_error(void);

#ifdef __cplusplus
}
#endif
#endif
