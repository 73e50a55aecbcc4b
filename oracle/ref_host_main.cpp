// ref_host_main.cpp -- TEST INFRASTRUCTURE: a command line over the REFERENCE's own host classes, compiled for
// Linux against oracle/win32_standin (oracle/Makefile, target `ref` -> oracle/_ref/ref_host).  It is what
// tests/golden/host_golden.json was recorded from (oracle/make_host_golden.py).
//
// One action per process, always started as a child (oracle.ref_host): the reference keeps its settings in
// statics, leaks, frees mpArkData twice when LoadArkData runs twice on one object (ExtractFiles calls it itself),
// and reads 4 bytes past its buffer at the end of CDtaFile::Load -- so this is never loaded into an interpreter and
// never built with a sanitizer.  All paths are used as given; the reference resolves part files and the header
// name against the working directory, so the caller picks that.
//
//   ref_host [--ps3] [--keep-existing] [--allow-new] [--pack-all] ACTION ARGS...
//     dump HDR                  Load; the parsed table as one line of JSON on stdout (names as hex)
//     resave HDR OUTDIR         Load, LoadArkData, SaveArk( OUTDIR, HDR )
//     extract HDR OUTDIR        Load, ExtractFiles( 0, GetNumFiles(), OUTDIR )
//     pack REFHDR INDIR OUTDIR  Load( REFHDR ); ConstructFromDirectory( INDIR ), BuildArk( INDIR ), SaveArk( OUTDIR, REFHDR )
//     dta-resave IN OUT         CDtaFile::Load, CDtaFile::Save
// Exit status: the eError ordinal the first failing call returned (0 = eError_NoError), 64 for a bad command line.
// The reference's private members are read for `dump` (built with -fno-access-control).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "CArk.h"
#include "CDtaFile.h"
#include "Error.h"
#include "Settings.h"

namespace
{
void PrintHex( const std::string& lText )
{
    std::printf( "\"" );
    for( unsigned char c : lText ) std::printf( "%02x", c );
    std::printf( "\"" );
}

int Dump( const char* lpHeader )
{
    CArk lArk;
    eError leError = lArk.Load( lpHeader );
    if( leError != eError_NoError ) return (int)leError;
    std::printf( "{\"arks\": [" );
    for( int ii = 0; ii < lArk.miNumArks; ++ii )
    {
        std::printf( "%s{\"size\": %u, \"path\": ", ii ? ", " : "", lArk.mpArks[ ii ].muSize );
        PrintHex( lArk.mpArks[ ii ].mPath );
        std::printf( "}" );
    }
    std::printf( "], \"files\": [" );
    for( int ii = 0; ii < lArk.miNumFiles; ++ii )
    {
        const auto& f = lArk.mpFiles[ ii ];
        std::printf( "%s{\"name\": ", ii ? ", " : "" );
        PrintHex( f.mName );
        std::printf( ", \"size\": %u, \"offset\": %lld, \"flags1\": %d, \"flags2\": %d, \"hash\": %u}", (unsigned)f.miSize,
                     (long long)f.mi64Offset, f.miFlags1, f.miFlags2, (unsigned)f.miHash );
    }
    std::printf( "]}\n" );
    return 0;
}

int Resave( const char* lpHeader, const char* lpOutDir )
{
    CArk lArk;
    eError leError = lArk.Load( lpHeader );
    if( leError != eError_NoError ) return (int)leError;
    leError = lArk.LoadArkData();
    if( leError != eError_NoError ) return (int)leError;
    return (int)lArk.SaveArk( lpOutDir, lpHeader );
}

int Extract( const char* lpHeader, const char* lpOutDir )
{
    CArk lArk;
    eError leError = lArk.Load( lpHeader );
    if( leError != eError_NoError ) return (int)leError;
    return (int)lArk.ExtractFiles( 0, lArk.GetNumFiles(), lpOutDir );
}

int Pack( const char* lpRefHeader, const char* lpInDir, const char* lpOutDir )
{
    CArk lReference;
    eError leError = lReference.Load( lpRefHeader );
    if( leError != eError_NoError ) return (int)leError;
    CArk lArk;
    leError = lArk.ConstructFromDirectory( lpInDir, lReference, std::vector< SSongConfig >() );
    if( leError != eError_NoError ) return (int)leError;
    leError = lArk.BuildArk( lpInDir, std::vector< SSongConfig >() );
    if( leError != eError_NoError ) return (int)leError;
    return (int)lArk.SaveArk( lpOutDir, lpRefHeader );
}

int DtaResave( const char* lpIn, const char* lpOut )
{
    CDtaFile lDta;
    eError leError = lDta.Load( lpIn );
    if( leError != eError_NoError ) return (int)leError;
    return (int)lDta.Save( lpOut );
}
} // namespace

int main( int argc, char** argv )
{
    int ii = 1;
    for( ; ii < argc && std::strncmp( argv[ ii ], "--", 2 ) == 0; ++ii )
    {
        const std::string lSwitch = argv[ ii ];
        if( lSwitch == "--ps3" ) { CSettings::mbPS4 = false; CSettings::msPlatform = "ps3"; }
        else if( lSwitch == "--keep-existing" ) CSettings::mbOverwriteOutputFiles = false;
        else if( lSwitch == "--allow-new" ) CSettings::mbIgnoreNewFiles = false;
        else if( lSwitch == "--pack-all" ) CSettings::mbPackAllFiles = true;
        else return 64;
    }
    if( ii >= argc ) return 64;
    const std::string lAction = argv[ ii++ ];
    const int liArgs = argc - ii;
    char** lpArgs = argv + ii;
    int liStatus = 64;
    if( lAction == "dump" && liArgs == 1 ) liStatus = Dump( lpArgs[ 0 ] );
    else if( lAction == "resave" && liArgs == 2 ) liStatus = Resave( lpArgs[ 0 ], lpArgs[ 1 ] );
    else if( lAction == "extract" && liArgs == 2 ) liStatus = Extract( lpArgs[ 0 ], lpArgs[ 1 ] );
    else if( lAction == "pack" && liArgs == 3 ) liStatus = Pack( lpArgs[ 0 ], lpArgs[ 1 ], lpArgs[ 2 ] );
    else if( lAction == "dta-resave" && liArgs == 2 ) liStatus = DtaResave( lpArgs[ 0 ], lpArgs[ 1 ] );
    std::fflush( stdout );
    return liStatus;
}
